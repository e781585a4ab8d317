"""Every element of the attention backward against an fp64 reference and a derived worst-case error bound (attn_bwd_reference.py):
yv_attention_bwd, yv_attention_bwd_long, yv_attention_bwd_short and yv_attention_cls_bwd, each on its own (the bit equality of the
long and short kernels with yv_attention_bwd lives in their own files and is not repeated), delta_ws, the out and lse of
yv_attention_train and the lse of yv_attention_cls_train, the memory past the live rows, and the isolation of a crop of
yv_attention_bwd from a NaN neighbour.  The operands (out, lse) are built on the CPU from the fp64 forward, so a backward kernel is
tested on its own.  The gate is |got - ref| <= 1.01 B for every element; test_attn_bwd_reference_cpu.py shows on the CPU that an
emulation of the kernels' arithmetic stays inside it and that a dropped row, a 1 % scale error, a zero delta and a wrong lse / delta
index fall outside.  Each test prints its worst |got - ref| / B; the module prints the worst per kernel and output at its end."""
import pytest
import torch

import attn_bwd_reference as ab
from attn_bwd_reference import GATE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL_ROWS, TAIL_FLOATS = -24576.0, 4, 64                   # bf16-representable; no gradient of these cases comes near it
WORST = {}                                                           # (kernel, output) -> (ratio, case)


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    yield yvhip
    print("\nworst |got - ref| / bound per kernel and output over the case list (gate 1.01):")
    for (kernel, output), (r, case) in sorted(WORST.items()):
        print(f"  attn-bound {kernel} {output} {r:.3f} at {case}")


def _note(kernel, output, r, case):
    if r > WORST.get((kernel, output), (-1.0, None))[0]:
        WORST[(kernel, output)] = (r, case)


def _dev(case, *names):
    return [case[n].to(DEV) for n in names]


def _run_bwd(fn, qkv, out, dout, lse, R, N, H):
    """-> (dqkv with TAIL_ROWS extra rows, delta_ws with TAIL_FLOATS extra floats), both pre-filled with the sentinel, on the CPU"""
    dqkv = torch.full((R * N + TAIL_ROWS, 3 * H * 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
    dws = torch.full((R * H * N + TAIL_FLOATS,), SENTINEL, device=DEV)
    fn(qkv, out, dout, lse, R, N, H, dqkv, dws)
    torch.cuda.synchronize()
    return dqkv.cpu(), dws.cpu()


def _where(row, col, R, N, H, D):
    """the element of a gradient third: crop, head, token, column of the head, and the 32-row group edge the token sits on"""
    tok = row % N
    edge = "first of a group" if tok % 32 == 0 else "last of a group" if tok % 32 == 31 else "last token" if tok == N - 1 else "inside"
    return f"crop {row // N} head {col // 64} token {tok} ({edge}) column {col % 64}"


# ------------------------------------------------------------------------------------------------ 1. the three full backward kernels
KERNELS = ("attention_bwd", "attention_bwd_long", "attention_bwd_short")
BWD_CASES = [(kern, *s, kind) for kern in KERNELS for s in ab.BWD_SHAPES for kind in ab.KINDS if kern != "attention_bwd_short" or s[1] <= 224]


@pytest.mark.parametrize("kernel,R,N,H,kind", BWD_CASES)
def test_attention_bwd_elementwise_bound(yv, kernel, R, N, H, kind):
    case = ab.bwd_case(R, N, H, kind)
    ref, D, M, FL = case["ref"], H * 64, R * N, R * H * N
    dqkv, dws = _run_bwd(getattr(yv, kernel), *_dev(case, "qkv", "out", "dout", "lse"), R, N, H)
    got = dqkv.float()
    assert bool((got[M:] == SENTINEL).all()) and bool((dws[FL:] == SENTINEL).all())          # nothing past row R*N / float R*H*N
    assert bool(torch.isfinite(got[:M]).all()) and bool(torch.isfinite(dws[:FL]).all())
    assert not bool((got[:M] == SENTINEL).any()) and not bool((dws[:FL] == SENTINEL).any())  # every live element overwritten
    r, where = ab.ratios(got[:M], ref, D)
    r["delta"], i = ab.worst(dws[:FL], ref["delta"], ref["b_delta"])
    tag = f"R={R} N={N} H={H} {kind}"
    print(f"{kernel} {tag}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        _note(kernel, k, v, tag)
    for k, v in r.items():
        at = f"crop {i // (H * N)} head {i // N % H} token {i % N}" if k == "delta" else _where(*where[k], R, N, H, D)
        assert v <= GATE, (kernel, k, v, at)


# ------------------------------------------------------------------------------------------------ 2. the forward that feeds them
@pytest.mark.parametrize("kind", ab.KINDS)
@pytest.mark.parametrize("R,N,H", ab.BWD_SHAPES)
def test_attention_train_elementwise_bound(yv, R, N, H, kind):
    case = ab.operands(R, N, H, kind)
    fwd, D, M, FL = case["fwd"], H * 64, R * N, R * H * N
    out = torch.full((M + TAIL_ROWS, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((FL + TAIL_FLOATS,), SENTINEL, device=DEV)
    yv.attention_train(case["qkv"].to(DEV), R, N, H, out, lse)
    torch.cuda.synchronize()
    out, lse = out.cpu().float(), lse.cpu()
    assert bool((out[M:] == SENTINEL).all()) and bool((lse[FL:] == SENTINEL).all())
    assert bool(torch.isfinite(out[:M]).all()) and bool(torch.isfinite(lse[:FL]).all())
    r_out, i = ab.worst(out[:M], fwd["out"], fwd["b_out"])
    r_lse, j = ab.worst(lse[:FL], fwd["lse"], fwd["b_lse"])
    tag = f"R={R} N={N} H={H} {kind}"
    print(f"attention_train {tag}: worst |got - ref| / bound out {r_out:.3f}, lse {r_lse:.3f}")
    _note("attention_train", "out", r_out, tag)
    _note("attention_train", "lse", r_lse, tag)
    assert r_out <= GATE, ("out", r_out, _where(i // D, i % D, R, N, H, D))
    assert r_lse <= GATE, ("lse", r_lse, f"crop {j // (H * N)} head {j // N % H} token {j % N}")


# ------------------------------------------------------------------------------------------------ 3. a NaN neighbour
@pytest.mark.parametrize("bad", [0, 1])
@pytest.mark.parametrize("R,N,H", [s for s in ab.BWD_SHAPES if s[0] == 2])
def test_attention_bwd_poisoned_neighbour(yv, R, N, H, bad):
    """The other crop's rows of qkv, out, dout and lse set to NaN: the clean crop's dqkv rows and delta keep their bits."""
    case = ab.bwd_case(R, N, H, "peaked")
    ins = _dev(case, "qkv", "out", "dout", "lse")
    clean, clean_d = _run_bwd(yv.attention_bwd, *ins, R, N, H)
    for t in ins[:3]:
        t[bad * N:(bad + 1) * N] = float("nan")
    ins[3][bad * H * N:(bad + 1) * H * N] = float("nan")
    got, got_d = _run_bwd(yv.attention_bwd, *ins, R, N, H)
    good = 1 - bad
    assert bool(torch.isfinite(clean[:R * N].float()).all())
    assert torch.equal(got[good * N:(good + 1) * N], clean[good * N:(good + 1) * N])
    assert torch.equal(got_d[good * H * N:(good + 1) * H * N], clean_d[good * H * N:(good + 1) * H * N])
    assert bool((got[R * N:].float() == SENTINEL).all()) and bool((got_d[R * H * N:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4. the cls-query kernels
@pytest.mark.parametrize("kind", ab.KINDS)
@pytest.mark.parametrize("R,N,H", ab.CLS_SHAPES)
def test_attention_cls_bwd_elementwise_bound(yv, R, N, H, kind):
    """yv_attention_cls_bwd under its f32-only bound (no bf16 operand cast), q the strided cls view, lse built on the CPU."""
    case = ab.cls_case(R, N, H, kind)
    ref, D, M = case["ref"], H * 64, R * N
    qd, dod, lse = _dev(case, "qkv", "dout", "lse")
    q = qd[::N, :D]
    assert q.stride(0) == N * 3 * D
    dqkv = torch.full((M + TAIL_ROWS, 3 * D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    yv.attention_cls_bwd(q, qd, dod, lse, R, N, H, dqkv)
    torch.cuda.synchronize()
    got = dqkv.cpu().float()
    assert bool((got[M:] == SENTINEL).all())
    assert bool(torch.isfinite(got[:M]).all()) and not bool((got[:M] == SENTINEL).any())
    other = torch.ones(M, dtype=torch.bool)
    other[::N] = False
    assert bool((got[:M][other][:, :D] == 0).all())                                          # the Q third of non-cls rows: exactly 0
    r, where = ab.ratios(got[:M], ref, D)
    tag = f"R={R} N={N} H={H} {kind}"
    print(f"attention_cls_bwd {tag}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        _note("attention_cls_bwd", k, v, tag)
    for k, v in r.items():
        assert v <= GATE, (k, v, _where(*where[k], R, N, H, D))


@pytest.mark.parametrize("kind", ab.KINDS)
@pytest.mark.parametrize("R,N,H", ab.CLS_SHAPES)
def test_attention_cls_train_lse_bound(yv, R, N, H, kind):
    """The lse of yv_attention_cls_train against the fp64 log2-sum-exp of query 0 under the lse bound of yv_attention_train (the flat
    1e-3 of test_gpu_cls_tail_train.py::test_attention_cls_train_forward stays where it is)."""
    case = ab.cls_case(R, N, H, kind)
    D = H * 64
    qd = case["qkv"].to(DEV)
    out = torch.full((R + TAIL_ROWS, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((R * H + TAIL_FLOATS,), SENTINEL, device=DEV)
    yv.attention_cls_train(qd[::N, :D], qd, R, N, H, out, lse)
    torch.cuda.synchronize()
    out, lse = out.cpu().float(), lse.cpu()
    assert bool((out[R:] == SENTINEL).all()) and bool((lse[R * H:] == SENTINEL).all())
    assert bool(torch.isfinite(out[:R]).all()) and bool(torch.isfinite(lse[:R * H]).all())
    r, i = ab.worst(lse[:R * H], case["lse64"], case["b_lse"])
    tag = f"R={R} N={N} H={H} {kind}"
    print(f"attention_cls_train {tag}: worst |lse - ref| / bound {r:.3f}")
    _note("attention_cls_train", "lse", r, tag)
    assert r <= GATE, ("lse", r, f"crop {i // H} head {i % H}")
