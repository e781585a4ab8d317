"""The gates of yolo_glue_reference.py proven on the CPU.  A (derived bounds): an f32 emulation of yv_bn_stats / yv_bn_act_fwd /
yv_bn_act_bwd in the kernels' own lane / chunk / finaliser order stays inside |got - ref| <= 1.01 B on every case
test_gpu_yolo_glue.py runs, and named wrong kernels fall outside on at least one case each; the emulation is bit-exact on the integer
cases.  B (exact kernels): the plain-indexing references agree with torch's own operators and differ from named wrong kernels on
the case list.  C (yv_detect_loss): the restated loss agrees in f32 with oracle.yolo_train.detection_loss, takes in f32 the
decisions it takes in f64 on every case (that is what the margins are for), differs from the named wrong tie rules, and the measured
constants behind K are pinned.  The host-side argument checks of the entry points are pinned through ctypes with host addresses
that are never dereferenced: only calls that return before any HIP call."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import yolo_glue_reference as yg
from yolo_glue_reference import GATE, worst

SMALL_BN_CASES = [c for c in yg.BN_CASES if c not in yg.BN_BIG]


# ------------------------------------------------------------------------------------------------ A: BatchNorm + SiLU
@functools.lru_cache(maxsize=None)
def _bn_ratios(case, mutant=None):
    """-> {output and options: worst |emulation - ref| / B}; the two large cases run one option set"""
    c = yg.bn_case(*case)
    mean, rstd = yg.bn_operand_stats(c["z"])
    big = case in yg.BN_BIG
    r = {}
    ref = yg.bn_stats_reference(c["z"], c["rm0"], c["rv0"])
    e = yg.emu_bn_stats(c["z"], c["rm0"], c["rv0"], mutant=mutant)
    for n in ("mean", "rstd", "run_mean", "run_var"):
        r["stats " + n] = worst(e[n], ref[n], ref["b_" + n])[0]
    for act, res in ([(1, True)] if big else yg.BN_OPTS):
        rs = c["res"] if res else None
        a, b = yg.bn_act_fwd_reference(c["z"], mean, rstd, c["gamma"], c["beta"], rs, act)
        got = yg.emu_bn_act_fwd(c["z"], mean, rstd, c["gamma"], c["beta"], rs, act, mutant)
        r[f"fwd a act={act} res={int(res)}"] = worst(got.float(), a, b)[0]
    for act, bs in ([(1, 1)] if big else yg.BN_BWD_OPTS):
        ref = yg.bn_act_bwd_reference(c["da"], c["z"], mean, rstd, c["gamma"], c["beta"], act, bs)
        dz, dga, dbe = yg.emu_bn_act_bwd(c["da"], c["z"], mean, rstd, c["gamma"], c["beta"], act, bs, mutant)
        for n, got in (("dz", dz.float()), ("dgamma", dga), ("dbeta", dbe)):
            r[f"bwd {n} act={act} bs={bs}"] = worst(got, ref[n], ref["b_" + n])[0]
    return r


@pytest.mark.parametrize("case", yg.BN_CASES, ids=str)
def test_bn_emulation_inside_gate(case):
    r = _bn_ratios(case)
    print(f"bn emulation {case}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= GATE, {k: v for k, v in r.items() if v > GATE}


BN_EXPECT = {"biased_running_var": ((1024, 2, "rand"), "stats run_var"), "dz_without_k2": ((24, 86, "rand"), "bwd dz act=1 bs=1"),
             "silu_without_u_term": ((8, 1, "rand"), "bwd dbeta act=1 bs=1"), "drop_chunk_last_row": ((8, 257, "rand"), "stats mean"),
             "drop_last_group": ((24, 85, "rand"), "fwd a act=0 res=0"), "res_before_rounding": ((8, 255, "rand"), "fwd a act=1 res=1")}


@pytest.mark.parametrize("mutant", yg.BN_MUTANTS)
def test_bn_mutants_outside_gate(mutant):
    case, output = BN_EXPECT[mutant]
    r = _bn_ratios(case, mutant)
    assert r[output] > GATE, f"{mutant} passes the gate at {case}: {r}"
    if mutant == "biased_running_var":                      # an error of the running variance only, and none at T = 1
        assert all(v <= GATE for k, v in r.items() if k != output) and max(_bn_ratios((1024, 1, "rand"), mutant).values()) <= GATE
    if mutant == "dz_without_k2":                           # frozen statistics have no such term
        assert r["bwd dz act=1 bs=0"] <= GATE and r["bwd dgamma act=1 bs=1"] <= GATE
    if mutant == "silu_without_u_term":
        assert all(v <= GATE for k, v in r.items() if "act=0" in k or k.startswith(("stats", "fwd")))
    if mutant == "res_before_rounding":                     # visible with a shortcut only
        assert all(v <= GATE for k, v in r.items() if "res=1" not in k)
    caught = [c for c in SMALL_BN_CASES if max(_bn_ratios(c, mutant).values()) > GATE]
    print(f"{mutant}: outside the gate on {len(caught)} of {len(SMALL_BN_CASES)} cases")
    assert case in caught


def test_bn_case_list_covers_the_edges():
    for Cn in (8, 24, 1024):
        rp = yg.row_lanes(Cn)
        ts = {T for c, T, k in yg.BN_CASES if c == Cn and k == "rand"}
        assert {1, max(rp - 1, 1), rp, rp + 1, 4 * rp - 1, 4 * rp, 4 * rp + 1, 16 * rp - 1, 16 * rp + 1, 257} <= ts, Cn
    assert yg.row_lanes(24) == 85 and yg.row_lanes(8) == 256 and yg.row_lanes(1024) == 2
    assert yg.chunks_for(8449) == (34, 249) and yg.chunks_for(524289) == (2041, 257) and yg.chunks_for(257) == (2, 129)
    assert {c for c, _, _ in yg.BN_CASES} == {8, 16, 24, 48, 256, 1024}


def test_bn_value_cases():
    """the constant channel has var 0 and rstd = 1 / sqrt(eps); the two large-mean channels: what the bound says rstd keeps"""
    for case in [c for c in yg.BN_CASES if c[2] == "values"]:
        z = yg.bn_case(*case)["z"]
        ref = yg.bn_stats_reference(z)
        assert float(ref["var"][0]) == 0.0 and abs(float(ref["rstd"][0]) - yg.f32v(yg.BN_EPS) ** -0.5) < 1e-12
        r8, a8 = yg.bn_stats_accuracy(z, yg.VALUE_CHANNELS["ratio8"])
        r64, a64 = yg.bn_stats_accuracy(z, yg.VALUE_CHANNELS["ratio64"])
        print(f"bn_stats accuracy {case}: |mean| / std {r8:.1f}: B_rstd / rstd {a8:.2e};  {r64:.1f}: {a64:.2e}")
        assert 7 < r8 < 9 and 60 < r64 < 70 and a8 < a64
        mean, rstd = yg.bn_operand_stats(z)
        c = yg.bn_case(*case)
        u = c["gamma"] * ((z - mean) * rstd) + c["beta"]
        assert float(u[:, 3].min()) > 28 and float(u[:, 4].max()) < -28             # the SiLU tails
    # the worst of the list: 256 row lanes added serially in f32 (C = 8) leave rstd a ninth of its value at |mean| / std = 64
    assert 0.05 < yg.bn_stats_accuracy(yg.bn_case(8, 257, "values")["z"], 2)[1] < 0.2


def test_bn_rstd_bound_is_not_linearised():
    """where the error of var exceeds var + eps the linearised d_var / (2 (var + eps)) is no bound; the interval form is"""
    z = torch.full((257, 8), 64.0) + torch.tensor([0.0, 0.5] * 128 + [0.0]).view(257, 1) * 0.03125
    z = yg.bf(z).float()
    ref = yg.bn_stats_reference(z, eps=1e-7)
    assert float(ref["d_var"][0]) > float(ref["var"][0]) + 1e-7
    assert bool(torch.isfinite(ref["b_rstd"]).all()) and float(ref["b_rstd"][0]) > 0.5 * float(ref["rstd"][0])
    e = yg.emu_bn_stats(z, eps=1e-7)
    assert worst(e["rstd"], ref["rstd"], ref["b_rstd"])[0] <= GATE


@pytest.mark.parametrize("case", [(8, 257), (24, 86), (1024, 33), (16, 8449), (8, 1)], ids=str)
def test_bn_emulation_exact_on_integers(case):
    Cn, T = case
    c = yg.bn_case(Cn, T, "rand", exact=True)
    e = yg.emu_bn_stats(c["z"], c["rm0"], c["rv0"])
    mean, rstd, rm, rv = yg.bn_stats_exact(c["z"], c["rm0"], c["rv0"])
    assert torch.equal(e["mean"], mean) and torch.equal(e["rstd"], rstd) and torch.equal(e["run_mean"], rm) and torch.equal(e["run_var"], rv)
    assert torch.equal(mean, (c["z"].double().sum(0) / T).float())
    one, mu = torch.ones(Cn), torch.ones(Cn)
    dz, _, dbeta = yg.emu_bn_act_bwd(c["da"], c["z"], mu, one, c["gamma"], c["beta"], act=0, batch_stats=0)
    assert torch.equal(dbeta, c["da"].sum(0)) and torch.equal(dz, yg.bf(2.0 * c["da"]))
    for mutant in ("drop_chunk_last_row", "drop_last_group"):
        assert not torch.equal(yg.emu_bn_act_bwd(c["da"], c["z"], mu, one, c["gamma"], c["beta"], 0, 0, mutant)[2], c["da"].sum(0))


def test_res_rounds_twice_on_exact_operands():
    """v = z + 2^-9 needs nine bits: bf16(bf16(v) + res) and bf16(v + res) differ on a lattice of 2^-9, and the emulation is the former"""
    g = torch.Generator().manual_seed(1)
    z = yg.int_tensor((86, 24), g, 1, 1)
    res = torch.randint(0, 8, (86, 24), generator=g).float() * 2.0 ** -9
    zero, one, beta = torch.zeros(24), torch.ones(24), torch.full((24,), 2.0 ** -9)
    got = yg.emu_bn_act_fwd(z, zero, one, one, beta, res, act=0)
    assert torch.equal(got, yg.bf(yg.bf(z + beta).float() + res))
    assert not torch.equal(got, yg.emu_bn_act_fwd(z, zero, one, one, beta, res, act=0, mutant="res_before_rounding"))


# ------------------------------------------------------------------------------------------------ B: exact kernels
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("H,W", yg.POOL_SHAPES)
def test_maxpool5_bwd_reference(H, W):
    """the plain-indexing reference is torch's own adjoint (first maximum in scan order); routing to the last differs on ties"""
    differs = False
    for pattern in yg.POOL_PATTERNS:
        c = yg.pool_case(H, W, 8, pattern)
        xr = _nchw(c["x"]).requires_grad_(True)
        F.max_pool2d(xr, 5, 1, 2).backward(_nchw(c["dout"]))
        ref = yg.maxpool5_bwd_reference(c["x"], c["dout"], c["din0"])
        assert torch.equal(ref, c["din0"] + _nhwc(xr.grad)) and float(ref.abs().max()) < 256
        wrong = yg.maxpool5_bwd_reference(c["x"], c["dout"], c["din0"], mutant="last_maximum")
        assert torch.equal(wrong, ref) == (pattern == "increasing" or H * W == 1)
        differs |= not torch.equal(wrong, ref)
    assert differs or H * W == 1


@pytest.mark.parametrize("B,H,W", yg.VIEW_SHAPES)
def test_view_op_reference(B, H, W):
    for mode in range(7):
        c = yg.view_case(mode, B, H, W, 8)
        ref = yg.view_op_reference(mode, c["src"], c["dst0"], H, W)
        assert float(ref.abs().max()) < 256
        s = c["src"]
        if mode == 2:
            assert torch.equal(ref, s.repeat_interleave(2, 1).repeat_interleave(2, 2))
        if mode == 3:
            assert torch.equal(ref, c["dst0"] + s.view(B, H, 2, W, 2, 8).sum((2, 4)))
        if mode == 4:
            exp = torch.zeros_like(ref)
            exp[:, ::2, ::2] = s
            assert torch.equal(ref, exp)
            assert not torch.equal(yg.view_op_reference(4, s, c["dst0"], H, W, mutant="zero_insert_odd"), ref)
        if mode == 6:
            assert torch.equal(ref, F.pad(s, (0, 0, 1, 1, 1, 1)))


@pytest.mark.parametrize("Hin,Win", yg.IM2COL_SHAPES)
@pytest.mark.parametrize("stride", [1, 2])
def test_im2col3_reference(Hin, Win, stride):
    x = yg.int_tensor((2, Hin, Win, 8), torch.Generator().manual_seed(Hin * 9 + Win))
    ref = yg.im2col3_reference(x, stride)
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    exp = F.unfold(_nchw(x), 3, padding=1, stride=stride).view(2, 8, 9, Hout * Wout).permute(0, 3, 2, 1).reshape(2 * Hout * Wout, 72)
    assert torch.equal(ref, exp)
    wrong = yg.im2col3_reference(x, stride, mutant="floor_out")
    assert (wrong.shape == ref.shape) == (stride == 1 or (Hin % 2 == 0 and Win % 2 == 0))       # odd sizes at stride 2 show it


def test_weight_dgrad_blob_sppf_references():
    w = yg.int_tensor((40, 9, 24), torch.Generator().manual_seed(3))
    assert torch.equal(yg.weight_dgrad_reference(w), w.flip(1).permute(2, 1, 0))
    for pixels in yg.BLOB_PIXELS:
        img = yg.blob_case(pixels)
        assert pixels == 1 or img.unique().numel() == 256
        out = yg.blob_reference(img)
        assert out.dtype == torch.bfloat16 and bool((out[:, 3:] == 0).all()) and bool((out[:, :3][img == 255] == 1.0).all())
    x = yg.int_tensor((2, 3, 7, 8), torch.Generator().manual_seed(4))
    ys = [_nchw(x)]
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
    assert torch.equal(yg.sppf_reference(x), _nhwc(torch.cat(ys, 1)))


# ------------------------------------------------------------------------------------------------ C: detection loss
@pytest.mark.parametrize("case", yg.ORACLE_CASES, ids=str)
def test_loss_reference_is_the_oracle_in_f32(case):
    """on the four random cases of test_gpu_yolo_train.py the restated loss, evaluated in f32, is oracle.yolo_train.detection_loss"""
    from oracle import yolo_train as oy
    B, S, G, counts, seed = case
    outs, box, cls, gtb, gtl, cnt = yg.oracle_case(*case)
    mask = torch.arange(G)[None] < cnt[:, None]
    total, parts = oy.detection_loss(outs, gtl.long(), gtb, mask, S, 5)
    total.backward()
    got = yg.detect_loss_reference(box, cls, gtb, gtl, cnt, S, 5, dtype=torch.float32)
    for v, r in zip(got["loss"], (total.detach(), *parts)):
        assert abs(float(v) - float(r)) <= 2e-5 * max(1.0, abs(float(r))), (got["loss"], total, parts)
    for s in range(3):
        rb = outs[s][0].grad if outs[s][0].grad is not None else torch.zeros_like(outs[s][0])
        rb, rc = rb.permute(0, 2, 3, 1).reshape(-1, 64), outs[s][1].grad.permute(0, 2, 3, 1).reshape(-1, 5)
        assert float((got["dbox"][s] - rb).abs().max()) <= 2e-5 * max(float(rb.abs().max()), 1e-30) or float(rb.abs().max()) == 0
        assert float((got["dcls"][s][:, :5] - rc).abs().max()) <= 2e-5 * float(rc.abs().max())
        assert bool((got["dcls"][s][:, 5:] == 0).all())
        assert torch.equal((got["dbox"][s] != 0).any(1), (rb != 0).any(1))                   # the same positives


@pytest.mark.parametrize("name", list(yg.LOSS_CASES))
def test_loss_case_margins_and_f32_decisions(name):
    c = yg.loss_case(name)                                   # asserts the lattice and finds a seed with every margin
    ref = c["ref"]
    print(f"loss case {name}: seed {c['seed']} positives {int((ref['tgt'] >= 0).sum())} margins {ref['margins']}")
    assert ref["ok"] and ref["margins"]["branch"] >= yg.BRANCH_MARGIN
    f32 = yg.detect_loss_reference(c["box"], c["cls"], c["gtb"], c["gtl"], c["cnt"], c["S"], c["nc"], dtype=torch.float32)
    assert torch.equal(f32["tgt"], ref["tgt"]) and torch.equal(f32["inside"], ref["inside"]) and torch.equal(f32["chosen"], ref["chosen"])
    assert torch.equal(f32["weight"] > 0, ref["weight"] > 0)
    rows = torch.cat([(d != 0).any(1).view(c["B"], -1) for d in ref["dbox"]], 1)              # `dbox row non-zero` is `fg and weight > 0`
    assert torch.equal(rows, (ref["tgt"] >= 0) & (ref["weight"] > 0))


def test_loss_case_list_properties():
    """what the list was built to contain is there"""
    n_in = lambda name: yg.loss_case(name)["ref"]["inside"].sum(-1)
    assert n_in("small")[0, :2].tolist() == [1, 0] and n_in("s32")[:, 0].tolist() == [15, 1]
    assert int(n_in("metric0")[0, 0]) > 10 and int(n_in("edges")[0, 0]) == 11
    c = yg.loss_case("metric0")
    assert sorted(torch.nonzero(c["ref"]["tgt"][0] >= 0).view(-1).tolist()) == torch.nonzero(c["ref"]["inside"][0, 0]).view(-1)[:10].tolist()
    assert float(c["ref"]["weight"].max()) == 0.0 and float(torch.cat(c["ref"]["dbox"]).abs().max()) == 0.0
    c = yg.loss_case("twins")
    shared = c["ref"]["chosen"][0, 0] & c["ref"]["chosen"][0, 1]
    assert int(shared.sum()) == 10 and bool((c["ref"]["tgt"][0][shared] == 0).all())
    c = yg.loss_case("edges")
    ax, ay, st = yg.anchors_of(64, torch.float64)
    on_edge = (st == 8) & ((ax * 8 == 4) | (ax * 8 == 36)) & (ay * 8 > 4) & (ay * 8 < 28)
    assert int(on_edge.sum()) == 4 and not bool(c["ref"]["inside"][0, 0][on_edge].any())
    c = yg.loss_case("s64")
    assert c["gtl"][0].tolist()[1:3] == [-3, 7] and c["cnt"].tolist() == [6, 0] and bool((c["ref"]["tgt"][1] == -1).all())
    for g in (1, 2):                                         # the clamped labels carry weight: class 0 and class nc - 1 get a target
        assert bool(((c["ref"]["tgt"][0] == g) & (c["ref"]["weight"][0] > 0)).any()), g
    c = yg.loss_case("s160")
    assert c["ref"]["margins"]["dfl_clamped"] > 0 and float(c["box"][0].max()) == 30.0 and float(c["cls"][0].min()) == -30.0
    assert (c["nc"], c["ncp"]) == (80, 80) and float(c["gtb"][0, 0, 2] - c["gtb"][0, 0, 0]) > 15 * 8
    c = yg.loss_case("empty")
    assert float(c["ref"]["loss"][1]) == 0.0 and float(torch.cat(c["ref"]["dbox"]).abs().max()) == 0.0
    assert yg.loss_case("s640")["A"] == 8400 and yg.loss_case("s32")["A"] == 21


@pytest.mark.parametrize("wrong,name", [({"ties": "descending"}, "metric0"), ({"claim": "last"}, "twins"), ({"inside": "ge"}, "edges")])
def test_loss_wrong_tie_rules_differ(wrong, name):
    c = yg.loss_case(name)
    got = yg.detect_loss_reference(c["box"], c["cls"], c["gtb"], c["gtl"], c["cnt"], c["S"], c["nc"], **wrong)
    assert not torch.equal(got["tgt"], c["ref"]["tgt"])
    blind = []                                               # the random cases that cannot tell: why the constructed ones are in the list
    for n in ("s64", "s160"):
        o = yg.loss_case(n)
        if torch.equal(yg.detect_loss_reference(o["box"], o["cls"], o["gtb"], o["gtl"], o["cnt"], o["S"], o["nc"], **wrong)["tgt"], o["ref"]["tgt"]):
            blind.append(n)
    print(f"{wrong}: seen on {name}; not seen on {blind}")


def test_loss_measured_constants():
    """K = 8 * max(1, M): M is measured here, on the CPU, from this file's formulas in f32; the pinned figures may not drift"""
    m = yg.measure_loss_m()
    print("measured |f32 - f64| / (EPS * scale):", {k: round(v, 2) for k, v in m.items()})
    for k in yg.LOSS_OUTPUTS:
        assert 0.5 * yg.LOSS_M[k] <= m[k] <= yg.LOSS_M[k], (k, m[k], yg.LOSS_M[k])
        assert yg.loss_k(k) == 8 * yg.LOSS_M[k] >= 8


def test_loss_workspace_rule():
    import yvhip
    for B, A, G in ((1, 21, 1), (2, 525, 6), (1, 8400, 6)):
        assert yvhip.detect_loss_ws_bytes(B, A, G) == yg.loss_ws_bytes(B, A, G)
        lay = yg.loss_ws_layout(B, A, G)
        assert (lay["tgt"][0] + lay["tgt"][1]) * 4 + 256 == yg.loss_ws_bytes(B, A, G)


# ------------------------------------------------------------------------------------------------ host argument checks
ARG, LIMIT, WORKSPACE = -1, -2, -3                          # YV_ERR_ARG, YV_ERR_LIMIT, YV_ERR_WORKSPACE (include/yv_hip.h)
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256           # a 256-byte aligned host address: never dereferenced


@pytest.fixture(scope="module")
def lib():
    import yvhip
    return yvhip.lib


def _vp(a):
    return C.c_void_p(a) if a else None


def _stats(lib, z=P, ld=32, T=100, Cn=24, rm=P, rv=P, short=1):
    return lib.yv_bn_stats(_vp(z), ld, T, Cn, 1e-3, 0.03, _vp(P), _vp(P), _vp(rm), _vp(rv), _vp(P), yg.bn_ws_floats(T, Cn) - short, None)


def _fwd(lib, z=P, ldz=32, T=100, Cn=24, res=0, ldres=32, out=P, ldo=32):
    return lib.yv_bn_act_fwd(_vp(z), ldz, T, Cn, _vp(P), _vp(P), _vp(P), _vp(P), _vp(res), ldres, _vp(out), ldo, 1, None)


def _bwd(lib, da=P, ldda=32, z=P, ldz=32, T=100, Cn=24, dz=P, lddz=32, short=1):
    return lib.yv_bn_act_bwd(_vp(da), ldda, _vp(z), ldz, T, Cn, _vp(P), _vp(P), _vp(P), _vp(P), 1, 1, _vp(P), _vp(P), _vp(dz), lddz, _vp(P),
                             yg.bn_ws_floats(T, Cn) - short, None)


def test_bn_argument_checks(lib):
    """every call here ends at a check: the plain call with a workspace one float short is YV_ERR_WORKSPACE, so each ARG below is
    decided before it"""
    assert _stats(lib) == WORKSPACE and _bwd(lib) == WORKSPACE
    for T, Cn in ((1, 8), (257, 8), (8449, 16), (524289, 8), (33, 1024)):
        assert int(lib.yv_bn_ws_floats(T, Cn)) == yg.bn_ws_floats(T, Cn)
        assert _stats(lib, T=T, Cn=Cn, ld=Cn) == WORKSPACE and _bwd(lib, T=T, Cn=Cn, ldda=Cn, ldz=Cn, lddz=Cn) == WORKSPACE
    for Cn in (1032, 12, 0):
        assert _stats(lib, Cn=Cn, ld=1040) == ARG and _fwd(lib, Cn=Cn, ldz=1040, ldo=1040) == ARG
        assert _bwd(lib, Cn=Cn, ldda=1040, ldz=1040, lddz=1040) == ARG
    assert _stats(lib, z=P + 8) == ARG and _stats(lib, ld=16) == ARG and _stats(lib, ld=36) == ARG and _stats(lib, T=0) == ARG
    assert _stats(lib, rm=0) == ARG and _stats(lib, rv=0) == ARG and _stats(lib, rm=0, rv=0) == WORKSPACE
    assert _fwd(lib, z=P + 8) == ARG and _fwd(lib, out=P + 2) == ARG and _fwd(lib, res=P + 8) == ARG
    assert _fwd(lib, ldz=16) == ARG and _fwd(lib, ldz=36) == ARG and _fwd(lib, ldo=16) == ARG and _fwd(lib, ldo=36) == ARG
    assert _fwd(lib, res=P, ldres=36) == ARG and _fwd(lib, res=P, ldres=16) == ARG            # the shortcut's stride too
    for name in ("da", "z", "dz"):
        assert _bwd(lib, **{name: P + 8}) == ARG, name
    for name in ("ldda", "ldz", "lddz"):
        assert _bwd(lib, **{name: 16}) == ARG and _bwd(lib, **{name: 36}) == ARG, name


def test_exact_kernel_argument_checks(lib):
    p = _vp(P)
    assert lib.yv_maxpool5_bwd(p, 8, p, 8, p, 8, 2, 3, 7, 8, p, 2 * 3 * 7 * 8 - 1, None) == WORKSPACE
    assert lib.yv_maxpool5_bwd(p, 8, p, 8, p, 8, 2, 3, 7, 12, p, 1 << 20, None) == ARG
    assert lib.yv_maxpool5_bwd(p, 8, p, 12, p, 8, 2, 3, 7, 8, p, 1 << 20, None) == ARG
    for lds in ((8, 16, 16), (16, 8, 16), (16, 16, 8)):     # a row stride below C: rows would overlap and the last one end past the view
        assert lib.yv_maxpool5_bwd(p, lds[0], p, lds[1], p, lds[2], 2, 3, 7, 16, p, 1 << 20, None) == ARG, lds
    assert lib.yv_im2col3(p, 8, 1, 5, 7, 16, 1, p, None) == ARG
    assert lib.yv_sppf_pool(p, 1, 41, 40, 32, 8, None) == LIMIT and lib.yv_sppf_pool(p, 1, 40, 40, 24, 8, None) == ARG
    assert lib.yv_view_op(7, p, 8, p, 8, 1, 1, 1, 8, None) == ARG and lib.yv_view_op(0, p, 8, p, 12, 1, 1, 1, 8, None) == ARG
    assert lib.yv_view_op(0, _vp(P + 8), 8, p, 8, 1, 1, 1, 8, None) == ARG and lib.yv_view_op(0, None, 8, p, 8, 1, 1, 1, 8, None) == ARG
    assert lib.yv_im2col3(p, 8, 1, 5, 7, 8, 3, p, None) == ARG and lib.yv_im2col3(p, 8, 1, 5, 7, 12, 1, p, None) == ARG
    assert lib.yv_conv_weight_dgrad(p, 3, 4, 5, p, None) == ARG and lib.yv_blob_nhwc8(p, 0, p, None) == ARG


def test_detect_loss_argument_checks(lib):
    arr = (C.c_void_p * 3)(P, P, P)
    p = _vp(P)
    call = lambda B=2, S=64, nc=5, ncp=8, G=6, ws=0: lib.yv_detect_loss(arr, arr, arr, arr, B, S, nc, ncp, p, p, p, G, 7.5, 0.5, 1.5, p, p, ws, None)
    assert call(ws=yg.loss_ws_bytes(2, 84, 6) - 1) == WORKSPACE
    assert call(S=48) == ARG and call(nc=81, ncp=88) == ARG and call(nc=5, ncp=4) == ARG and call(G=0) == ARG and call(B=0) == ARG
