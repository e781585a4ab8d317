"""VitTrainer's launch order, pinned on the CPU: the calls the trainer makes (native wrappers, stream and event operations, torch's own
kernels, the reducer), their operands and their streams over two steps equal tests/golden/vit_trainer_trace.json call by call.  The
fixture was recorded (tests/trainer_trace.py --write) before the trainer's blocks were folded into one body per direction; the same
calls on the same operands on the same streams in the same order compute the same bits."""
import os

import pytest

import trainer_trace


@pytest.fixture(scope="module")
def fixture():
    return trainer_trace.load_fixture()


def test_fixture_holds_exactly_the_cases(fixture):
    assert list(fixture) == list(trainer_trace.CASES)
    assert os.path.getsize(trainer_trace.FIXTURE) < os.path.getsize(os.path.join(trainer_trace.HERE, "golden", "golden.json"))


@pytest.mark.parametrize("case", list(trainer_trace.CASES))
def test_trainer_trace_equals_fixture(fixture, case):
    got, want = trainer_trace.record_case(case), fixture[case]
    assert got["allocs"] == want["allocs"]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if g != w:
            pytest.fail(f"{case}: call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(got["calls"]) == len(want["calls"]), \
        f"{case}: {len(got['calls'])} calls recorded, {len(want['calls'])} in the fixture; first extra: " \
        f"{(got['calls'] + want['calls'])[min(len(got['calls']), len(want['calls']))]}"


def test_the_trace_holds_what_it_must(fixture):
    """What makes the fixture worth comparing against: both steps, both streams, the cross-block wait, torch's own kernels."""
    calls = fixture["bf16"]["calls"]
    names = [c[0] for c in calls]
    one_step = names[:names.index("sgd_step")]
    assert (one_step.count("aten.copy_"), one_step.count("aten.clone"), one_step.count("aten.zero_")) == (5, 2, 1)
    assert [c[3].get("first", False) for c in calls if c[0] == "sgd_step"] == [True, False]
    assert {c[1] for c in calls if c[0] == "wgrad"} == {0, 1}                     # head / patch-embed on main, blocks on the side stream
    waits = [c[2][1] for c in calls if c[0] == "stream.wait_event" and c[2][0] == ["stream", 0]]
    records = [c[2][0] for c in calls if c[0] == "event.record" and c[2][1] == ["stream", 1]]
    assert waits[0] == records[0]                                                 # step 1, block 0 waits on block 2's weight gradients
    assert len(waits) == 1 + 3 and len(records) == 6
    for case, attn in (("bf16", {"attention_train", "attention_bwd"}), ("bf16_p8_long", {"attention_long", "attention_bwd_long"}),
                       ("mxfp8_cls_tail", {"attention_train", "attention_bwd", "attention_cls_train", "attention_cls_bwd"}),
                       ("mxfp8_cls_tail_p8_long", {"attention_long", "attention_bwd_long", "attention_cls_train", "attention_cls_bwd"})):
        assert {c[0] for c in fixture[case]["calls"] if c[0].startswith("attention")} == attn, case
