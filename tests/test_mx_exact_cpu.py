"""The exact-integer gate of the MXFP8 forward kernels (mx_exact.py, test_gpu_mx_exact.py) proved without a device: the builders'
preconditions hold for every case, every case takes the route it names (yv_linear_route and yv_conv2d_mxfp8_instance are host
only), every kernel instance the route functions can answer has a case, and a plain emulation of each product from the quantised
bytes and scales equals the reference while each planted addressing fault changes the output - a fault of the scale addressing
nearly all of it, so that the exponent pattern and not a planted block is what sees it."""
import functools

import pytest
import torch

import mx_exact as mx
import yvhip as yv

LIN = {c["name"]: c for c in mx.lin_cases(yv)}
CONV = {c["name"]: c for c in mx.conv_cases()}


@functools.lru_cache(maxsize=None)
def conv_data(name):
    return mx.conv_data(CONV[name])


# ---------------------------------------------------------------------------------------------------------- preconditions
def test_form_constants_are_the_measured_ones():
    """FORM_ERR records form_errors() rounded up (at most 1 % above), and the erfc form gives exactly 0.5 at 0."""
    got = mx.form_errors()
    for k, v in mx.FORM_ERR.items():
        assert got[k] <= v <= 1.01 * got[k], (k, got[k], v)
    assert float(mx.gelu_grad_form(torch.zeros(1))[0]) == 0.5


@pytest.mark.parametrize("shape", sorted(mx.LIN_SHAPES))
def test_linear_builder_preconditions(shape):
    d = mx.lin_data(shape)                                         # asserts (a) survives the quantiser, (b) < 2^24, the planted blocks
    assert torch.equal(d["lin"], d["lin"].round()) and not bool((d["lin"] == mx.SENTINEL).any())
    assert d["mag"] < 2 ** 24 and d["K"] % 128 == 0
    cnt, mul = mx.M_DEV[shape]
    assert 0 < cnt * mul < d["M"] and (cnt * mul) % 32                 # the device row count cuts inside a tile
    assert bool((d["u"][:, mx.AUX_ZERO_COL] == 0).all()) and float(d["u"].abs().max()) <= mx.FORM_RANGE["gelu_grad"]
    assert torch.equal(mx.bf(d["u"]).float(), d["u"])
    # bf16 rounding is exercised: some exact sums are not bf16 values
    assert bool((mx.bf(d["lin"]).float() != d["lin"]).any())


@pytest.mark.parametrize("name", sorted(CONV))
def test_conv_builder_preconditions(name):
    c, d = CONV[name], conv_data(name)
    assert torch.equal(d["ref"], d["ref"].round()) and d["kreal"] == c["k"] ** 2 * c["cin"]
    for x in d["bufs"]:                                            # loud borders in every channel of the buffer
        for edge, sign in ((x[:, 0, :-1], 1), (x[:, :-1, 0], 1), (x[:, -1], -1), (x[:, :, -1], -1)):
            assert float((edge * sign >= 2).float().mean()) > 0.9      # (all but a planted block)
    for (off, ld), spare in ((c["out"], 8), (c["res"], 0)):
        assert off % 8 == 0 and ld % 8 == 0 and ld >= off + c["cout"] + spare   # 16-byte aligned: the staged rule; spare channels
    once = mx.bf(d["ref"] + d["res"][..., c["res"][0]:c["res"][0] + c["cout"]])
    assert bool((once != mx.conv_expected(c, d, "res")).any())     # the shortcut's two rounding rules differ on this case


# ------------------------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("name", sorted(LIN))
def test_linear_case_takes_the_route_it_names(name):
    c = LIN[name]
    N = mx.LIN_SHAPES[c["shape"]][1]
    with mx.options(yv, linear_p8_rows=c["rows"]):
        for form, flags, kw in mx.family_queries(yv, c["fam"], N):
            assert mx.lin_route(yv, c, flags, **kw) == c["expect"], (name, form)


@pytest.mark.parametrize("name", sorted(CONV))
def test_conv_case_takes_the_instance_it_names(name):
    assert mx.conv_instance(yv, CONV[name]) == CONV[name]["inst"]


def test_every_reachable_instance_has_a_case():
    """Every (kernel, tile_rows, f32out, ext) yv_linear_route(mx=1) answers over the bench shapes, the cases' shapes and the
    thresholds of the rule, under the shipped options and under every forced height, is the route of an exact case; so are both
    instances of the convolution over every MX-eligible layer of the three detector scales."""
    covered = {c["expect"] for c in LIN.values()}
    B, G, R, O, PRE, GB = yv.EPI_BIAS, yv.EPI_GELU, yv.EPI_RES_F32, yv.EPI_OUT_F32, yv.EPI_SAVE_PRE, yv.EPI_GELU_BWD
    forms = [(B, {}), (B | G, {}), (B | O, {}), (B | R, {}), (B | R, dict(res_f32=True)), (B | G | PRE, "aux"), (GB, "aux"),
             (B, dict(m_dev=True))]
    seen = set()
    for rows in (0, 96, 100, 128, 160, 192, 224, 256):
        with mx.options(yv, linear_p8_rows=rows):
            for M in (64, 197, 1000, 2047, 2048, 2085, 6304, 12608, 25216):
                for N in (128, 136, 768, 1024, 2304, 3072, 3584, 4096, 4352):
                    for K in (128, 256, 384, 640, 768, 1024, 3072, 4096):
                        for flags, kw in forms:
                            kw = dict(ldaux=N) if kw == "aux" else kw
                            r = yv.linear_route(M, N, K, flags, mx=True, n_cu=256, **kw)
                            assert r.mx == 1
                            seen.add((r.kernel, r.tile_rows, r.f32out, r.ext))
    assert seen <= covered, sorted(seen - covered)
    assert seen == covered, sorted(covered - seen)                 # and no case names a route the rule cannot answer
    assert len({k for k, _, _, _ in seen}) == 2 and len(seen) == 15
    from oracle import yolo
    from yvhip.engines import LAYER_STRIDE
    inst = set()
    for scale, Bt in (("n", 32), ("s", 16), ("m", 64)):
        for key, cin, cout, k, s in yolo.conv_shapes(scale, 5):
            if cin % 32 or cout % 32:
                continue
            parts = key.split(".")
            idx = int(parts[1])
            H = 640 // ((8, 16, 32)[int(parts[3])] if idx == 22 else LAYER_STRIDE[idx])
            inst.add(yv.conv2d_mxfp8_instance(Bt, H, H, k, s, cin, cout))
    assert inst == {0, 1} == {c["inst"] for c in CONV.values()}


def test_each_conv_instance_has_every_addressing_form():
    for inst in (0, 1):
        cs = [c for c in CONV.values() if c["inst"] == inst]
        npix = lambda c: c["B"] * c["H"] * c["W"]
        assert any(c["k"] == 3 and c["s"] == 1 for c in cs) and any(c["k"] == 3 and c["s"] == 2 for c in cs)
        assert any(len(c["srcs"]) == 2 and c["srcs"][0][0] % 128 and not c["srcs"][0][1] for c in cs)      # boundary inside a K step
        assert any(len(c["srcs"]) == 2 and c["srcs"][0][1] == 1 for c in cs)                                # upsampled first source
        assert any(c["srcs"][0][2] > 0 and c["srcs"][0][3] > c["srcs"][0][0] for c in cs)                   # offset, stride > C
        assert any(c["H"] == 2 and c["W"] == 2 for c in cs) and any(npix(c) % 128 for c in cs)              # 2 x 2 image, ragged M
        assert any((c["k"] ** 2 * c["cin"]) % 128 for c in cs)                                              # a zero-padded K tail
        assert all(npix(c) > 128 or c["H"] == 2 for c in cs)


# ------------------------------------------------------------------------------------------------------------------ faults
def assert_seen(ref, bad, rows, fault, what):
    """A fault of the scale addressing (mx.SCALE_FAULTS) must change the output nearly everywhere - at least 90 % of the values,
    99 % of the rows and 99 % of the columns - so that it is the exponent PATTERN that sees it in every tile, lane and column, not
    the three planted blocks.  Any other fault changes only the part of the output it touches: at least one value."""
    ch = (bad != ref).reshape(rows, -1)
    vals, r, c = float(ch.float().mean()), float(ch.any(1).float().mean()), float(ch.any(0).float().mean())
    if fault in mx.SCALE_FAULTS:
        assert vals >= 0.9 and r >= 0.99 and c >= 0.99, (what, fault, vals, r, c)
    else:
        assert vals > 0, (what, fault)


def test_patterns_differ_between_all_neighbours():
    """Scale bytes of the linear operands: rows m / m + 1 differ in every block, and the four blocks of every K step are distinct
    (outside the planted blocks); the same for the convolution weight, and for a map along y, x and the channel blocks."""
    from mx_reference import emulate_quant_rows
    d = mx.lin_data("s300")
    for t in (d["a"], d["w"]):
        s = emulate_quant_rows(t)[1].int()
        assert float((s[1:] != s[:-1]).float().mean()) > 0.97
        steps = s.view(s.shape[0], -1, 4)
        assert float((steps.sort(-1)[0].diff(dim=-1) > 0).all(-1).float().mean()) > 0.97
    c = CONV["t64_3x3_kpad"]
    s = emulate_quant_rows(conv_data(c["name"])["bufs"][0])[1].int()
    for dim in (1, 2, 3):
        assert float((s.narrow(dim, 1, s.shape[dim] - 1) != s.narrow(dim, 0, s.shape[dim] - 1)).float().mean()) > 0.97, dim


@pytest.mark.parametrize("shape", sorted(mx.LIN_SHAPES))
def test_linear_emulation_equals_the_reference_and_sees_every_fault(shape):
    d = mx.lin_data(shape)
    assert torch.equal(mx.lin_emulate(d), d["lin"])
    for fault in mx.LIN_FAULTS:
        assert_seen(d["lin"], mx.lin_emulate(d, fault), d["M"], fault, shape)


@pytest.mark.parametrize("name", sorted(CONV))
def test_conv_emulation_equals_the_reference_and_sees_every_fault(name):
    c, d = CONV[name], conv_data(name)
    assert torch.equal(mx.conv_emulate(c, d), d["ref"])
    for fault in mx.CONV_FAULTS:
        if not mx.conv_fault_applies(c, fault):
            continue
        bad = mx.conv_emulate(c, d, fault)
        assert bad.shape == d["ref"].shape
        assert_seen(d["ref"], bad, c["B"] * c["H"] * c["W"], fault, name)


def test_every_fault_applies_somewhere_in_each_instance():
    for inst in (0, 1):
        for fault in mx.CONV_FAULTS:
            assert any(mx.conv_fault_applies(c, fault) for c in CONV.values() if c["inst"] == inst), (inst, fault)
