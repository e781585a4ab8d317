"""The launch lists of YoloEngine and VitEngine, pinned on the CPU: the calls every engine configuration makes (native wrappers
with their operands, option changes, torch's own kernels) equal tests/golden/engine_trace.json call by call.  The fixture was
recorded (tests/engine_trace.py --write) before the engines' launch lists were folded into one spelling each; the same calls on the
same operands in the same order compute the same bits.  One case was recorded afterwards: yolo_n5_mxfp8_unfused, the fused_c2f flip
on an mxfp8 engine, which raised before; it is pinned against the cases that were."""
import os

import pytest

import engine_trace
import trainer_trace


@pytest.fixture(scope="module")
def fixture():
    return engine_trace.load_fixture()


def _names(calls):
    return [c[0] for c in calls]


def test_fixture_holds_exactly_the_cases(fixture):
    assert list(fixture) == engine_trace.CASES
    assert os.path.getsize(engine_trace.FIXTURE) < os.path.getsize(os.path.join(trainer_trace.HERE, "golden", "golden.json"))


@pytest.mark.parametrize("case", engine_trace.CASES)
def test_engine_trace_equals_fixture(fixture, case):
    got, want = engine_trace.record_case(case), fixture[case]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{case}: call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(got) == len(want), \
        f"{case}: {len(got)} calls recorded, {len(want)} in the fixture; first extra: {(got + want)[min(len(got), len(want))]}"


def test_the_trace_holds_what_it_must(fixture):
    """What makes the fixture worth comparing against: each case took the path it is named for."""
    fused = {"yolo_n5_bf16": 2, "yolo_n80_bf16": 2, "yolo_n5_mxfp8": 2, "yolo_n5_bf16_forward_raw": 2, "yolo_s5_mxfp8": 1}
    for case in engine_trace.YOLO_CASES:                # n: model.2 and model.4 are fused blocks, s: model.2, m: none; unfused: none
        names = _names(fixture[case])
        assert names[0] == "stem_conv" and names.count("sppf_pool") == 1, case
        assert ("conv2d_mxfp8" in names and "quant_mxfp8_map" in names) == ("mxfp8" in case), case
        assert names.count("c2f_fused") == fused.get(case, 0), case
    assert _names(fixture["yolo_n5_bf16"])[-1] == "detect_tail"
    assert _names(fixture["yolo_n80_bf16"])[-1] == "detect_decode"
    assert _names(fixture["yolo_n5_bf16_forward_raw"])[-6:] == ["aten.clone"] * 6
    two = [c for c in fixture["yolo_m5_mxfp8"] if c[2][1:2] != [None] and c[0].startswith("conv2d")]
    assert [c[0] for c in two] == ["conv2d"] * 4 and [c[2][0][3] for c in two] == [1, 1, 0, 0]  # the neck's concats (1 x 1: never MX),
    #                                                                                             two behind an upsampled source
    bf16_m2 = [c for c in fixture["yolo_m5_mxfp8"] if c[0] == "conv2d" and c[2][7].startswith("w.model.2.")]
    assert len(bf16_m2) == 2 + 2 * 2                                                            # the c = 48 block stays bf16
    for case in engine_trace.VIT_CASES:
        calls = fixture[case]
        names = _names(calls)
        assert "cls_rows" in names[:3] and names[-1] == "wrapper_head", case
        assert ("attention_long" in names) == ("long" in case), case
        assert ("attention" in names) == ("long" not in case and ("mxfp8" not in case or "attn_unfused" in case)), case
        assert ("quant_mxfp8" in names) == (case == "vit_mxfp8_attn_unfused"), case
        assert ("linear_res_ln" in names) == case.endswith("_ln"), case
        full = "_full" in case and "cus" not in case
        assert ("attention_cls" in names) == ("mxfp8" not in case and not full), case
        if full:                                        # cls_tail=False: the pass sits between the option's save / clear and its restore
            assert [c[:1] + c[2] for c in calls[:2]] == [["get_option", "linear_skinny"], ["set_option", "linear_skinny", 0]]
            assert names[2] == "cls_rows" and names[-3:] == ["linear", "set_option", "wrapper_head"]
            assert calls[-2][2] == ["linear_skinny", 1] and names.count("set_option") == 2
        else:
            assert "get_option" not in names, case
    long_mx = [c for c in fixture["vit_p8_mxfp8_long"] if c[0] == "attention_long"]
    assert len(long_mx) == 3 and all(c[3] == {"out_q": "q", "out_scale": "qs"} for c in long_mx)
    assert fixture["vit_p8_mxfp8_long_attn_unfused"] == fixture["vit_p8_mxfp8_long"]             # attention_long writes the operand itself
    calls = fixture["vit_bf16_full_cus_from_1"]
    at = [i for i, c in enumerate(calls) if c[0] == "set_option"]
    qkv = [i for i, c in enumerate(calls) if c[0] == "linear" and c[2][1].endswith("wqkv")]
    assert len(at) == 1 and calls[at[0]][2] == ["linear_p8_cus", 0] and qkv[0] < at[0] < qkv[1]  # behind block 0, in front of block 1
    uses_count = lambda c: len(c) > 3 and "count" in c[3].values()
    assert all(uses_count(c) for c in fixture["vit_bf16_count"] if c[0] != "cls_rows")
    assert not any(uses_count(c) for c in fixture["vit_bf16_tail"])


def test_fused_c2f_flip_on_an_mxfp8_engine(fixture):
    """eng.fused_c2f = False on an mxfp8 engine: outside model.2 / model.4 the launches of the mxfp8 case, inside them those of
    the unfused bf16 engine, each followed by the MX map of what it produced where an MX convolution reads it."""
    inside = lambda c: any(str(v).startswith(("w.model.2.", "w.model.4.")) for v in c[2]) or \
        (c[0] == "quant_mxfp8_map" and c[2][0] in ("out2", "out4", "y2", "y4", "t2", "t4"))
    split = lambda calls: ([c for c in calls if not inside(c)], [c for c in calls if inside(c) and c[0] != "quant_mxfp8_map"])
    flip_out, flip_in = split(fixture["yolo_n5_mxfp8_unfused"])
    mx_out, mx_in = split(fixture["yolo_n5_mxfp8"])
    _, bf16_in = split(fixture["yolo_n5_bf16_unfused"])
    assert flip_out == mx_out
    assert [c[0] for c in mx_in] == ["c2f_fused"] * 2
    assert flip_in == bf16_in and len(flip_in) == (2 + 2 * 1) + (2 + 2 * 2)
