"""YoloEngine(grouped_head=True) on the CPU: the recorded calls equal tests/golden/engine_trace_grouped.json, the head is
conv2d_group lines, and with every group expanded to its members the engine makes the convolution calls of the ungrouped engine
(tests/golden/engine_trace.json), argument for argument."""
import collections
import json

import pytest

import engine_trace
import engine_trace_grouped as etg


@pytest.fixture(scope="module")
def fixture():
    return etg.load_fixture()


@pytest.fixture(scope="module")
def ungrouped():
    return engine_trace.load_fixture()


def test_fixture_holds_exactly_the_cases(fixture):
    assert list(fixture) == list(etg.CASES)


@pytest.mark.parametrize("case", list(etg.CASES))
def test_trace_equals_fixture(fixture, case):
    got, want = etg.record_case(case), fixture[case]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{case}: call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(got) == len(want)


@pytest.mark.parametrize("case", list(etg.CASES))
def test_head_is_grouped_and_makes_the_ungrouped_engines_calls(fixture, ungrouped, case):
    calls, base = fixture[case], ungrouped[etg.CASES[case][1]]
    mx = "mxfp8" in case
    head = ("w.det", "w.model.22.", "wq.det", "wq.model.22.")
    is_head = lambda c: c[0] in ("conv2d", "conv2d_mxfp8") and str(c[2][7]).startswith(head)
    groups = [c for c in calls if c[0] == "conv2d_group"]
    # fused tail: two steps.  bf16: 3 + 6 members; mxfp8 (n): det1.0 and det2.0 are MXFP8 convolutions and run alone
    assert [len(c[2][0]) for c in groups] == ([1, 6] if mx else [3, 6])
    grouped_weights = {m[7] for c in groups for m in c[2][0]}
    assert not any(c[0] == "conv2d" and c[2][7] in grouped_weights for c in calls), "a grouped member also runs alone"
    assert [c[2][7] for c in calls if is_head(c)] == (["wq.det1.0.0", "wq.det2.0.0"] if mx else [])
    # everything in front of the head is the ungrouped engine's, call for call
    first = next(i for i, c in enumerate(calls) if c[0] == "conv2d_group" or is_head(c))
    assert calls[:first] == base[:first]
    assert calls[-1] == base[-1] and calls[-1][0] == "detect_tail"
    # ... and the convolution calls are the same multiset, argument for argument
    key = lambda c: json.dumps(c, sort_keys=True)
    convs = lambda cs: collections.Counter(key(c) for c in cs if c[0] in ("conv2d", "conv2d_mxfp8"))
    assert convs(etg.expand(calls)) == convs(base)
    other = lambda cs: collections.Counter(key(c) for c in cs if c[0] not in ("conv2d", "conv2d_mxfp8", "conv2d_group"))
    assert other(calls) == other(base)                                   # (the MX maps of what the head produced included)
    assert len(base) - len(calls) == sum(len(c[2][0]) - 1 for c in groups)
