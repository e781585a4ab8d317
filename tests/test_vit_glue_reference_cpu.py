"""The gate of vit_glue_reference.py proven on the CPU: for every bound, (a) an f32 emulation of the kernel's arithmetic in the
kernel's own order stays inside |got - ref| <= 1.01 B on every case of the list test_gpu_vit_glue.py runs, and (b) named wrong
kernels ("mutants" of the emulation) fall outside it on at least one case - so the bounds are neither too tight for a correct
kernel nor so wide that a subtle error passes.  The same file pins the host-side argument checks of the glue entry points through
ctypes with made-up non-null pointers: only calls that must return before any HIP call (as test_abi_cpu.py does)."""
import ctypes as C

import pytest
import torch

import vit_glue_reference as vg
from vit_glue_reference import GATE


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_run(kind, rows, cols, mutant=None, accumulate=False, ld=None, aligned=True):
    c = vg.colsum_case(kind, rows, cols)
    start = c["start"] if accumulate else None
    L, G = vg.colsum_path(kind, cols, ld, aligned)
    ref, bound = vg.colsum_reference(c["x"], start)
    return vg.worst(vg.emu_colsum(c["x"], L, G, start, mutant), ref, bound)[0]


@pytest.mark.parametrize("kind,rows,cols", vg.COLSUM_CASES)
def test_colsum_emulation_inside_gate(kind, rows, cols):
    for accumulate in (False, True):
        assert _colsum_run(kind, rows, cols, accumulate=accumulate) <= GATE
    if kind == "cast" and cols % 4 == 0:
        assert _colsum_run(kind, rows, cols, aligned=False) <= GATE            # the scalar cast forced by a misaligned x
    if kind == "bf16" and cols % 8 == 0:
        assert _colsum_run(kind, rows, cols, ld=cols + 4) <= GATE              # the scalar kernel forced by the row stride


@pytest.mark.parametrize("kind,rows,cols", vg.COLSUM_CASES)
def test_colsum_emulation_exact_on_integers(kind, rows, cols):
    c = vg.colsum_case(kind, rows, cols, exact=True)
    L, G = vg.colsum_path(kind, cols)
    for l, g in ((L, G), (1, 8), (1, G)):
        assert torch.equal(vg.emu_colsum(c["x"], l, g, c["start"]), (c["x"].double().sum(0) + c["start"].double()).float())


@pytest.mark.parametrize("mutant", vg.COLSUM_MUTANTS)
def test_colsum_mutants_outside_gate(mutant):
    caught = [(k, r, c) for k, r, c in vg.COLSUM_CASES if _colsum_run(k, r, c, mutant, accumulate=True) > GATE]
    assert caught, f"{mutant}: inside the gate on every case"
    expect = {"drop_block_last_row": ("cast", 32, 260), "drop_lane_tail": ("bf16", 33, 264), "ignore_accumulate": ("cast", 1, 4)}[mutant]
    assert expect in caught, f"{mutant} must be caught at {expect}; caught at {caught}"
    if mutant != "ignore_accumulate":                      # and on the exact integer data, where the check is equality
        k, r, c = expect
        ci = vg.colsum_case(k, r, c, exact=True)
        assert not torch.equal(vg.emu_colsum(ci["x"], *vg.colsum_path(k, c), None, mutant), ci["x"].sum(0))


def test_rne_bits_case_covers_the_boundaries():
    x = vg.rne_bits_case(33, 8)
    bits = x.view(torch.int32).reshape(-1) & 0xffff
    assert int((bits == 0x8000).sum()) > 30 and int((bits == 0x7fff).sum()) > 5 and int((bits == 0x8001).sum()) > 5
    assert bool(torch.isinf(x).any()) and not bool(torch.isnan(x).any())
    y = vg.bf(x).float()
    assert bool(torch.isinf(y[~torch.isinf(x)]).any())                        # the largest finite f32 rounds to infinity
    assert float(y.reshape(-1)[8]) == 1.0 and float(y.reshape(-1)[9]) == 1.015625     # 0x3f808000 ties down, 0x3f818000 up (to even)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd_ratio(case, mutant=None):
    c = vg.ln_case(*case)
    ref, bound = vg.ln_fwd_reference(c["x"], c["gamma"], c["beta"])
    return vg.worst(vg.emu_ln_fwd(c, mutant).float(), ref, bound)[0]


def _ln_bwd_ratios(case, mutant=None, G=32):
    c = vg.ln_case(*case)
    ref = vg.ln_bwd_reference(c["x"], c["gamma"], c["dy"], c["dx0"])
    dx, dga, dbe = vg.emu_ln_bwd(c, mutant, G)
    return {n: vg.worst(got, ref[n], ref["b_" + n])[0] for n, got in (("dx", dx), ("dgamma", dga), ("dbeta", dbe))}


@pytest.mark.parametrize("case", vg.LN_FWD_CASES, ids=str)
def test_layernorm_fwd_emulation_inside_gate(case):
    r = _ln_fwd_ratio(case)
    print(f"layernorm emulation {case}: {r:.3f}")
    assert r <= GATE


@pytest.mark.parametrize("case", vg.LN_BWD_CASES, ids=str)
def test_layernorm_bwd_emulation_inside_gate(case):
    for G in (32, 8):                                      # both second stages (8: the workspace that is not 16-byte aligned)
        r = _ln_bwd_ratios(case, G=G)
        print(f"layernorm_bwd emulation {case} G={G}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= GATE, r


def test_layernorm_bwd_dbeta_exact_on_integers():
    for D, rows in ((260, 9), (128, 1037)):
        c = dict(vg.ln_case(D, rows, "plain"))
        dy = vg.int_tensor((rows, D), torch.Generator().manual_seed(D))
        c["dy"], c["dybuf"] = vg.bf(dy), vg.bf(torch.cat([dy, torch.full((vg.NAN_ROWS, D), float("nan"))]))
        for G in (32, 8):
            assert torch.equal(vg.emu_ln_bwd(c, None, G)[2], dy.sum(0))


LN_FWD_EXPECT = {"eps_1e-5": (128, 9, "lowvar"), "var_over_d_minus_1": (4, 70, "plain"), "gamma_chunk_shift": (768, 70, "plain"),
                 "ignore_ldx": (192, 5, "strided")}
LN_BWD_EXPECT = {"eps_1e-5": (128, 9, "lowvar"), "var_over_d_minus_1": (4, 70, "plain"), "gamma_chunk_shift": (768, 70, "plain"),
                 "drop_m2": (192, 9, "plain"), "dgamma_from_g_gamma": (260, 70, "plain"), "ignore_ldx": (192, 9, "strided"),
                 "ignore_lddy": (1024, 9, "strided")}


@pytest.mark.parametrize("mutant", vg.LN_MUTANTS_FWD)
def test_layernorm_fwd_mutants_outside_gate(mutant):
    case = LN_FWD_EXPECT[mutant]
    assert _ln_fwd_ratio(case, mutant) > GATE, f"{mutant} passes the gate at {case}"
    if mutant == "eps_1e-5":                               # visible on the low-variance case only: that is why it is in the list
        assert all(_ln_fwd_ratio(c, mutant) <= GATE for c in vg.LN_FWD_CASES if c[2] == "plain" and c[1] <= 5)


@pytest.mark.parametrize("mutant", vg.LN_MUTANTS_BWD)
def test_layernorm_bwd_mutants_outside_gate(mutant):
    case = LN_BWD_EXPECT[mutant]
    r = _ln_bwd_ratios(case, mutant)
    assert max(r.values()) > GATE, f"{mutant} passes the gate at {case}: {r}"
    if mutant == "dgamma_from_g_gamma":
        assert r["dgamma"] > GATE and r["dx"] <= GATE and r["dbeta"] <= GATE, r


# ------------------------------------------------------------------------------------------------ wrapper-head backward
@pytest.mark.parametrize("case", vg.HEAD_CASES, ids=str)
def test_head_bwd_emulation_inside_gate(case):
    c = vg.head_case(*case)                                # asserts the ReLU margin
    got = vg.emu_head_bwd(c)
    for n in ("dw1", "db1", "dw2", "db2", "dfeats"):
        r = vg.worst(got[n].float(), c["ref"][n], c["ref"]["b_" + n])[0]
        print(f"head_bwd emulation {case} {n}: {r:.3f}")
        assert r <= GATE, (n, r)


def test_head_bwd_mutant_outside_gate():
    """a backward that forgets the hidden ReLU mask, and one that passes gradient through features equal to zero"""
    c = vg.head_case(9, 5, 1024, 1024)
    f = c["feats"][:, :vg.HB_FEAT]
    rf = torch.relu(f)
    dh = c["dl"] @ c["w2"]                                                            # no (h > 0)
    assert vg.worst(dh.sum(0), c["ref"]["db1"], c["ref"]["b_db1"])[0] > GATE
    h = torch.relu(rf @ c["w1"].T + c["b1"])
    df = vg.bf(((c["dl"] @ c["w2"]) * (h > 0)) @ c["w1"] * (f >= 0))                  # >= for >
    assert vg.worst(df.float(), c["ref"]["dfeats"], c["ref"]["b_dfeats"])[0] > GATE


# ------------------------------------------------------------------------------------------------ loss
LOSS_CASES = [(B, nc, *w) for B, nc in vg.LOSS_SHAPES for w in vg.LOSS_WEIGHTS]


def _loss_ratios(B, nc, w_ls, w_fo, mutant=None):
    c = vg.loss_case(B, nc, w_ls, w_fo)
    loss, grad = vg.emu_loss(c["logits"], c["labels"], w_ls, w_fo, mutant)
    ref = c["ref"]
    return vg.worst(loss.reshape(1), ref["loss"].reshape(1), ref["b_loss"].reshape(1))[0], vg.worst(grad, ref["grad"], ref["b_grad"])[0]


@pytest.mark.parametrize("B,nc,w_ls,w_fo", LOSS_CASES)
def test_loss_emulation_inside_gate(B, nc, w_ls, w_fo):
    rl, rg = _loss_ratios(B, nc, w_ls, w_fo)
    print(f"loss emulation B={B} nc={nc} w=({w_ls:.3f}, {w_fo:.3f}): loss {rl:.3f} grad {rg:.3f}")
    assert rl <= GATE and rg <= GATE


@pytest.mark.parametrize("mutant", vg.LOSS_MUTANTS)
def test_loss_mutants_outside_gate(mutant):
    case = {"smoothing_0.11": (5, 5, 1.0, 0.0), "focal_mean_over_b": (5, 5, 0.0, 1.0), "drop_om": (257, 5, 1.0 / 6.0, 5.0 / 6.0)}[mutant]
    rl, rg = _loss_ratios(*case, mutant)
    assert rg > GATE, f"{mutant} passes the gradient gate at {case}"
    if mutant != "drop_om":                                # drop_om is an error of the derivative only
        assert rl > GATE, f"{mutant} passes the loss gate at {case}"


def test_loss_reference_domain():
    """The f32 form of the reference is finite at +-40 and infinite at +-80 (-log(softmax) underflows): the cases stay at +-30."""
    from oracle import train as ot
    t = torch.tensor([[1.0, 0.0]])
    assert bool(torch.isfinite(ot.build_loss(torch.tensor([[-40.0, 40.0]]), t)))
    assert not bool(torch.isfinite(ot.build_loss(torch.tensor([[-80.0, 80.0]]), t)))
    assert vg.LOGIT_RANGE == 30.0


# ------------------------------------------------------------------------------------------------ SGD
def test_sgd_reference_is_the_oracle_in_f32():
    from oracle import train as ot
    g = torch.Generator().manual_seed(0)
    p, gr, m = torch.randn(37, generator=g), torch.randn(37, generator=g), torch.randn(37, generator=g)
    pn, mn, mir = vg.sgd_reference(p, gr, torch.full((37,), float("nan")), 1e-3, 1.0 / 3.0, True)
    assert bool(torch.isfinite(pn).all()) and bool(torch.isfinite(mn).all())          # first: m is not read
    scaled = gr * torch.tensor(1.0 / 3.0, dtype=torch.float32)
    assert torch.equal(mn, scaled + torch.tensor(1e-3, dtype=torch.float32) * p) and torch.equal(mir, vg.bf(pn))
    pe, me = ot.sgd_step(p, gr, m, 1e-3)
    pn, mn, _ = vg.sgd_reference(p, gr, m, 1e-3, 1.0, False)
    assert torch.equal(pn, pe) and torch.equal(mn, me)


# ------------------------------------------------------------------------------------------------ host argument checks
ARG, LIMIT = -1, -2                                        # YV_ERR_ARG, YV_ERR_LIMIT (include/yv_hip.h)


@pytest.fixture(scope="module")
def lib():
    import yvhip
    return yvhip.lib


def _ptr(addr=0x10000):
    return C.c_void_p(addr)


def _ln(lib, x=0x10000, gamma=0x20000, beta=0x30000, y=0x40000, D=128, ldx=128, ldy=128):
    return lib.yv_layernorm(_ptr(x), ldx, _ptr(gamma), _ptr(beta), 4, D, 1e-6, _ptr(y), ldy, None, 1, None)


def _lnb(lib, x=0x10000, gamma=0x20000, dy=0x30000, dx=0x40000, D=128, ldx=128, lddy=128, lddx=128):
    return lib.yv_layernorm_bwd(_ptr(x), ldx, _ptr(gamma), _ptr(dy), lddy, 4, D, 1e-6, _ptr(dx), lddx, _ptr(0x50000), _ptr(0x60000),
                                _ptr(0x70000), None)


def test_layernorm_argument_checks(lib):
    assert _ln(lib, D=130) == ARG and _ln(lib, ldx=130) == ARG and _ln(lib, ldy=130) == ARG
    assert _ln(lib, D=1028, ldx=1028, ldy=1028) == LIMIT
    for name in ("x", "gamma", "beta"):                    # float4 reads: 16 bytes
        for off in (4, 8):
            assert _ln(lib, **{name: 0x10000 + off}) == ARG, (name, off)
    assert _ln(lib, y=0x40004) == ARG                      # uint2 stores: 8 bytes
    assert _ln(lib, D=1028, ldx=1028, ldy=1028, x=0x10004) == ARG             # the argument error comes first


def test_layernorm_bwd_argument_checks(lib):
    assert _lnb(lib, D=130) == ARG and _lnb(lib, ldx=130) == ARG and _lnb(lib, lddy=130) == ARG and _lnb(lib, lddx=130) == ARG
    assert _lnb(lib, D=1028, ldx=1028, lddy=1028, lddx=1028) == LIMIT
    for name in ("x", "gamma", "dx"):
        for off in (4, 8):
            assert _lnb(lib, **{name: 0x10000 + off}) == ARG, (name, off)
    assert _lnb(lib, dy=0x30004) == ARG and _lnb(lib, dy=0x30002) == ARG
    assert _lnb(lib, D=1028, ldx=1028, lddy=1028, lddx=1028, dx=0x40008) == ARG


def test_loss_head_sgd_argument_checks(lib):
    p = _ptr()
    assert lib.yv_loss_fwd_bwd(p, p, 4, 33, 1.0, 1.0, p, p, None) == LIMIT
    assert lib.yv_loss_fwd_bwd(p, p, 0, 5, 1.0, 1.0, p, p, None) == ARG
    assert lib.yv_head_bwd(p, 1000, p, p, p, p, 4, 33, p, p, p, p, p, 1000, p, None) == ARG
    assert lib.yv_head_bwd(p, 999, p, p, p, p, 4, 5, p, p, p, p, p, 1000, p, None) == ARG
    assert lib.yv_head_bwd(p, 1000, p, p, p, p, 4, 5, p, p, p, p, p, 999, p, None) == ARG
    for which in range(3):                                 # p, g, m: float4 accesses
        a = [0x10000, 0x20000, 0x30000]
        a[which] += 4
        assert lib.yv_sgd_step(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), 8, 1e-3, 0.9, 1e-3, 1.0, 0, None, None) == ARG, which
    assert lib.yv_sgd_step(p, p, p, 0, 1e-3, 0.9, 1e-3, 1.0, 0, None, None) == 0                  # nothing to do: no launch
