"""The saturated-SiLU gate of silu_exact.py without a device: every case of test_gpu_silu_exact.py builds and meets its
conditions, the f32 sums are order-free (shown, not assumed), and each planted fault changes the reference - the geometric ones
on a tile seam or an image border of the case - so the gate CAN fail."""
import pytest
import torch
import torch.nn.functional as F

import silu_exact as se

BIG = se.C2F_STRIDED_SHAPE                     # (2, 21, 37): 2 x 3 tiles, ragged both ways, two images


def big(c, n):
    return se.build_c2f(c, n, *BIG)


def changed(case, other):
    """Mask (B, H, W) of the pixels on which `other` differs from the case's reference."""
    return (other != case["ref"]).any(-1)


def on_seam(case, mask):
    return bool((mask & se.seam_mask(case["H"], case["W"])).any())


def test_bf16_round_is_round_to_nearest_even():
    """The float64 rounding written out in silu_exact.py against torch's own f32 -> bf16 cast: ties (x.5 steps), both signs, zero,
    and every 2^-4 step of the cases' range."""
    v = torch.arange(-(2 ** 16), 2 ** 16 + 1, dtype=torch.float64) / 16.0
    assert torch.equal(se.bf16_round(v), v.float().to(torch.bfloat16).double())
    ties = torch.tensor([257.0, 259.0, 24.0625, 24.1875, 513.0, 514.0, 518.0])          # halfway between two bf16 values
    assert se.bf16_round(ties).tolist() == [256.0, 260.0, 24.0, 24.25, 512.0, 512.0, 520.0]


@pytest.mark.parametrize("args", se.c2f_cases(), ids=lambda a: se.c2f_name(*a))
def test_c2f_case_builds_and_is_order_free(args):
    """Conditions (a) - (d) hold (the builder raises otherwise), and every layer's sum evaluated in FLOAT32, K forwards and K
    backwards, rounds to the bits of the float64 reference - for both rounding rules of the shortcut."""
    case = se.build_c2f(*args)
    st = case["stats"]
    assert st["min_pre"] >= se.FLOOR and st["bits"] < 24 and st["rules_differ"] > 0
    assert case["ref"].shape == (case["B"], case["H"], case["W"], 2 * case["c"])
    for staged in (False, True):
        out, layers = se.c2f_chain(case["x"], case["w"], case["b"], case["c"], case["n"], staged=staged)
        for i, lay in enumerate(layers):
            want = lay["pre"]
            if lay["res"] is not None:
                want = (se.bf16_round(want) if staged else want) + lay["res"]
            want = se.bf16_round(want)
            for reverse in (False, True):
                acc = se.sum_f32_ordered(lay["inp"], lay["w"], lay["k"], 1, reverse).view(lay["sum"].shape)
                got = acc + case["b"][i].view(1, -1, 1, 1)                              # f32 throughout, as the kernels
                if lay["res"] is not None:
                    got = (got.to(torch.bfloat16).float() if staged else got) + lay["res"].float()
                assert torch.equal(got.to(torch.bfloat16).double(), want), (case["name"], lay["name"], staged, reverse)


@pytest.mark.parametrize("args", se.stem_cases(), ids=lambda a: se.stem_name(*a))
def test_stem_case_builds_and_is_order_free(args):
    case = se.build_stem(*args)
    assert args[2] % 128 == 0 and case["stats"]["min_pre"] >= se.FLOOR and case["stats"]["bits"] < 24
    x = case["img"].permute(0, 3, 1, 2)
    w = (case["w"] * (1.0 / 255.0)).t().contiguous()                                  # f32 product, as stem_mfma_kernel forms it
    for reverse in (False, True):
        acc = se.sum_f32_ordered(x, w, 3, 2, reverse).view(case["B"], case["cout"], case["H"] // 2, case["W"] // 2)
        got = (acc + case["b"].view(1, -1, 1, 1)).to(torch.bfloat16).double().permute(0, 2, 3, 1)
        assert torch.equal(got, case["ref"]), (case["name"], reverse)


def test_grid_stride_case_has_more_chunks_than_slots():
    B, H, W, _ = se.STEM_GRID_STRIDE
    chunks = B * (H // 2) * (W // 2) // 64
    assert chunks == 8200 and se.STEM_GRID_SLOTS == 8192 and (chunks + 3) // 4 > 2048


def test_padded_form_of_the_chain_is_the_chain():
    """The block on a zero-extended image with its out-of-image intermediates masked equals the plain form (what fault b edits)."""
    for c, n in se.C2F_INSTANCES:
        case = big(c, n)
        assert torch.equal(se.c2f_reference(case, pad=2 * n + 1, masked=True), case["ref"])


# ------------------------------------------------------------------------------------------------ C2f faults
@pytest.mark.parametrize("c,n", se.C2F_INSTANCES)
def test_c2f_fault_a_two_taps_swapped(c, n):
    case = big(c, n)
    for layer in range(1, 1 + 2 * n):
        for t0, t1 in ((0, 1), (3, 5), (1, 7)):
            w = [t.clone() for t in case["w"]]
            w4 = w[layer].view(c, 9, c)
            w4[:, [t0, t1]] = w4[:, [t1, t0]]
            out = se.c2f_chain(case["x"], w, case["b"], c, n)[0]
            m = changed(case, out)
            assert float(m.double().mean()) > 0.9, (layer, t0, t1)
            assert on_seam(case, m)


@pytest.mark.parametrize("c,n", se.C2F_INSTANCES)
def test_c2f_fault_b_out_of_image_intermediates_kept(c, n):
    case = big(c, n)
    m = changed(case, se.c2f_reference(case, pad=2 * n + 1, masked=False))
    H, W = case["H"], case["W"]
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0] = border[-1] = True; border[:, 0] = border[:, -1] = True
    assert bool((m & border).any())
    assert not bool(m[:, 2 * n:H - 2 * n, 2 * n:W - 2 * n].any())                      # and nowhere the halo cannot reach
    for small in ((1, 1, 1), (1, 3, 5)):                                                # images smaller than the halo: everywhere
        cs = se.build_c2f(c, n, *small)
        assert bool(changed(cs, se.c2f_reference(cs, pad=2 * n + 1, masked=False)).all())


@pytest.mark.parametrize("c,n", se.C2F_INSTANCES)
def test_c2f_fault_c_halo_one_pixel_short(c, n):
    """Every tile of the case from its own halo of 2 n pixels IS the reference; from 2 n - 1 pixels its rim towards a neighbouring
    tile is not, and its interior still is."""
    case = big(c, n)
    H, W = case["H"], case["W"]
    for b in range(case["B"]):
        for ty in range((H + 15) // 16):
            for tx in range((W + 15) // 16):
                want = case["ref"][b, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
                assert torch.equal(se.c2f_tile_reference(case, b, ty, tx, 2 * n), want), (b, ty, tx)
                m = (se.c2f_tile_reference(case, b, ty, tx, 2 * n - 1) != want).any(-1)
                assert bool(m.any()), (b, ty, tx)
                rim = torch.zeros_like(m)
                rim[0] = rim[-1] = True; rim[:, 0] = rim[:, -1] = True
                assert bool((m & rim).any()) and not bool((m & ~rim).any()), (b, ty, tx)


@pytest.mark.parametrize("c,n", se.C2F_INSTANCES)
def test_c2f_fault_d_shortcut_from_the_wrong_array(c, n):
    case = big(c, n)
    for j in range(n):
        out = se.c2f_reference(case, shortcut_from=lambda i, j=j: i if i == j else i + 1)      # y(j) instead of y(j+1)
        assert float(changed(case, out).double().mean()) > 0.9, j


@pytest.mark.parametrize("args", se.c2f_cases(), ids=lambda a: se.c2f_name(*a))
def test_c2f_fault_e_shortcut_rounded_by_the_staged_rule(args):
    case = se.build_c2f(*args)
    assert not torch.equal(case["ref_staged"], case["ref"])                            # (condition d, every case)


@pytest.mark.parametrize("c,n", se.C2F_INSTANCES)
def test_c2f_fault_f_cv2_sources_in_another_order(c, n):
    case = big(c, n)
    for order in ([1, 0] + list(range(2, n + 2)), list(range(n + 1, -1, -1)), list(range(1, n + 2)) + [0]):
        out = se.c2f_reference(case, cv2_order=order)
        assert float(changed(case, out).double().mean()) > 0.9, order


@pytest.mark.parametrize("args", [a for a in se.c2f_cases() if a[2] > 1], ids=lambda a: se.c2f_name(*a))
def test_c2f_fault_g_one_image_for_another(args):
    case = se.build_c2f(*args)
    assert float((case["ref"][0] != case["ref"][1]).any(-1).double().mean()) > 0.5


# ------------------------------------------------------------------------------------------------ stem faults
def stem_small():
    return se.build_stem(2, 4, 256, 16)


def test_stem_fault_a_one_byte_shift():
    case = stem_small()
    flat = case["img"].reshape(case["B"], -1)
    for shifted in (torch.cat([flat[:, 1:], flat[:, :1] * 0], 1), torch.cat([flat[:, :1] * 0, flat[:, :-1]], 1)):
        out = se.stem_reference(case, img=shifted.reshape(case["img"].shape))
        assert float((out != case["ref"]).any(-1).double().mean()) > 0.9


def padded(case, left_from_previous_row=False, top=1):
    x = F.pad(case["img"].double().permute(0, 3, 1, 2), (1, 1, top, 2 - top))
    if left_from_previous_row:
        x[:, :, top + 1:top + case["H"], 0] = x[:, :, top:top + case["H"] - 1, case["W"]]      # the byte run in front of a row's start
    return x


def stem_from_padded(case, x):
    s = se.conv64(x, (case["w"].double() / 255.0).t().contiguous(), 3, stride=2, padding=0)
    return se.bf16_round(s + case["b"].double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)


def test_stem_fault_b_left_padding_from_the_previous_row():
    case = stem_small()
    assert torch.equal(stem_from_padded(case, padded(case)), case["ref"])              # the emulation itself
    m = (stem_from_padded(case, padded(case, left_from_previous_row=True)) != case["ref"]).any(-1)
    assert bool(m[:, 1:, 0].all()) and not bool(m[:, :, 1:].any())                     # the left column of every row but the first


def test_stem_fault_c_top_padding_dropped():
    case = stem_small()
    m = (stem_from_padded(case, padded(case, top=0)) != case["ref"]).any(-1)
    assert bool(m[:, 0].all()) and float(m.double().mean()) > 0.9


def test_stem_fault_d_chunk_seam():
    """The first pixel of a 64-pixel chunk taken from the previous chunk: its result is the one of the pixel to its left."""
    case = stem_small()
    assert case["W"] // 2 > 64
    out = case["ref"].clone()
    out[:, :, 64] = case["ref"][:, :, 63]
    m = (out != case["ref"]).any(-1)
    assert bool(m[:, :, 64].all())
    zero_left = padded(case)                                                            # ... or its left neighbour read as padding
    zero_left[:, :, :, 2 * 64] = 0
    m = (stem_from_padded(case, zero_left) != case["ref"]).any(-1)
    assert bool(m[:, :, 64].all())
