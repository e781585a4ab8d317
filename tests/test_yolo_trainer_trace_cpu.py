"""YoloTrainer's launch order, pinned on the CPU: the calls the trainer makes (native wrappers with every view's offset, shape and
row pitch, stream and event operations, torch's own kernels, the reducer) and their streams equal the fixtures under
tests/golden/yolo_trainer_trace/ call by call.  The fixtures were recorded (tests/yolo_trainer_trace.py --write) before the trainer's
wiring was folded into one launch list walked in both directions.  Activation gradients accumulate in bf16 into shared slices, so
the same calls on the same operands on the same streams in the same order is what computes the same bits."""
import os

import pytest

import trainer_trace
import yolo_trainer_trace as ytt


@pytest.fixture(scope="module")
def fixture():
    return ytt.load_fixture()


def _names(calls):
    return [c[0] for c in calls]


def _steps(calls):
    """The calls of each step: a step begins with the forward's first launch."""
    starts = [i for i, c in enumerate(calls) if c[0] == "blob_nhwc8"]
    assert starts[0] == 0
    return [calls[a:b] for a, b in zip(starts, starts[1:] + [len(calls)])]


def test_fixture_holds_exactly_the_cases(fixture):
    assert list(fixture) == sorted(ytt.CASES) and sorted(os.listdir(ytt.FIXTURE_DIR)) == sorted(c + ".json" for c in ytt.CASES)
    limit = os.path.getsize(os.path.join(trainer_trace.HERE, "golden", "golden.json"))
    for case in ytt.CASES:
        assert os.path.getsize(ytt.fixture_path(case)) < limit, case
    assert [len(_steps(fixture[case]["calls"])) for case in ytt.CASES] == [steps for steps, _ in ytt.CASES.values()]


@pytest.mark.parametrize("case", list(ytt.CASES))
def test_yolo_trainer_trace_equals_fixture(fixture, case):
    got, want = ytt.record_case(case), fixture[case]
    assert got["allocs"] == want["allocs"]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if g != w:
            pytest.fail(f"{case}: call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(got["calls"]) == len(want["calls"]), \
        f"{case}: {len(got['calls'])} calls recorded, {len(want['calls'])} in the fixture; first extra: " \
        f"{(got['calls'] + want['calls'])[min(len(got['calls']), len(want['calls']))]}"


def test_the_trace_holds_what_it_must(fixture):
    """What makes the fixtures worth comparing against: each case took the paths it is named for."""
    from yvhip import VIEW_PAD, VIEW_ZERO_INSERT
    stream_ops = ("stream.enter", "stream.exit", "stream.wait_event", "stream.wait_stream", "event.record")
    zero_inserts = lambda calls: [c for c in calls if c[0] == "view_op" and c[2][0] == VIEW_ZERO_INSERT]

    calls = fixture["default"]["calls"]
    # the weight gradients - wgrad, wgrad_conv3 and what fills their operands (_wgrad_block: the padded grids and their tail rows,
    # the im2col of the stride-2 blocks) - are on stream 1 and nowhere else, everything else is on stream 0
    wgrad_path = lambda c: c[0] in ("wgrad", "wgrad_conv3", "im2col3") or (c[0] == "view_op" and c[2][0] == VIEW_PAD) or \
        (c[0] == "aten.zero_" and c[2][0].startswith(("dzp", "col")))
    assert {c[1] for c in calls} == {0, 1}
    assert all(c[1] == (1 if wgrad_path(c) else 0) for c in calls if c[0] not in stream_ops)
    assert {"wgrad", "wgrad_conv3"} <= {c[0] for c in calls if c[1] == 1}
    assert [c[3].get("first", False) for c in calls if c[0] == "sgd_step"] == [True] * 3 + [False] * 3      # w, bnw, bias
    for step in _steps(calls):
        names = _names(step)
        assert names.count("event.record") == 3 + 16 and names.count("stream.wait_stream") == 1          # 3 head scales + 16 layers
        assert names.count("conv_dgrad_s2") == 0 and len(zero_inserts(step)) == 6
        assert "bn_stats" in names and "conv_view_stats" not in names and "im2col3" in names              # im2col3: the stride-2 blocks

    calls = fixture["all_optins"]["calls"]
    names = _names(calls)
    assert "conv_view_stats" in names and "bn_stats_finish" in names and "bn_stats" not in names
    assert names.count("conv_view_stats") == names.count("bn_stats_finish") == names.count("bn_act_fwd")
    assert names.count("conv_dgrad_s2") == 5
    assert [c[2][1] for c in zero_inserts(calls)] == ["dz.model.1"]                # the one stride-2 block the route leaves on zero insertion
    assert all(c[3].get("tile_n") == 0 for c in calls if c[0] in ("wgrad", "wgrad_conv3"))

    calls = fixture["serial_im2col_adamw_ema"]["calls"]
    names = _names(calls)
    assert not set(names) & set(stream_ops) and {c[1] for c in calls} == {0}
    assert "wgrad_conv3" not in names and names.count("wgrad") == names.count("conv_weight_dgrad") + 1   # + 1: the stem has no data gradient
    assert names.count("optim_step") == 3 and names.count("ema_update") == 2 and "sgd_step" not in names
