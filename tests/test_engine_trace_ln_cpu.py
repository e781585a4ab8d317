"""VitEngine(ln_gemm=True) on the CPU: the recorded calls equal tests/golden/engine_trace_ln.json; per full block the engine
records two linear_ln calls with the operands of the layernorm + linear pair they replace and no layernorm but the cls tail's and
the final one; with each linear_ln expanded to its pair and the option lines set aside, the trace is the engine's without the
flag (tests/golden/engine_trace.json), call for call.  Flag unset, or the environment variable on an engine that ignores it: that
golden case unchanged.  An explicit ln_gemm=True with fused_ln or dtype "mxfp8" raises."""
import pytest

import engine_trace
import engine_trace_ln as etl
import trainer_trace as tt


@pytest.fixture(scope="module")
def fixture():
    return etl.load_fixture()


@pytest.fixture(scope="module")
def base():
    return engine_trace.load_fixture()


def _is_ln_option(c):
    return c[0] in ("get_option", "set_option") and c[2][0] == "linear_ln_mid"


def test_fixture_holds_exactly_the_cases(fixture):
    assert list(fixture) == list(etl.CASES)


@pytest.mark.parametrize("case", list(etl.CASES))
def test_trace_equals_fixture(fixture, case):
    got, want = etl.record_case(case), fixture[case]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{case}: call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(got) == len(want)


@pytest.mark.parametrize("case", list(etl.CASES))
def test_linear_ln_stands_for_the_pair(fixture, base, case):
    from yvhip import engines
    model, kw, _, _, base_case = etl.CASES[case]
    calls, want = fixture[case], base[base_case]
    D, L = tt.MODELS[model][1], tt.MODELS[model][2]
    full = L if kw.get("cls_tail") is False else L - 1          # blocks run in full (cls_tail defaults to True)
    fused = [c for c in calls if c[0] == "linear_ln"]
    assert len(fused) == 2 * full
    for i in range(full):                                        # norm1 -> qkv, then norm2 -> fc1, on the residual stream
        a, b = fused[2 * i][2], fused[2 * i + 1][2]
        assert a == ["x", f"blocks.{i}.n1w", f"blocks.{i}.n1b", "h", f"blocks.{i}.wqkv", f"blocks.{i}.bqkv", "qkv"]
        assert b == ["x", f"blocks.{i}.n2w", f"blocks.{i}.n2b", "h", f"blocks.{i}.wfc1", f"blocks.{i}.bfc1", "g"]
    norms = [c[2][1] for c in calls if c[0] == "layernorm"]
    assert norms == ([] if full == L else [f"blocks.{L - 1}.n1w", f"blocks.{L - 1}.n2w"]) + ["nw"]
    # the pass sits between the option's save / set and its restore, outermost
    assert [c[:1] + c[2] for c in calls[:2]] == [["get_option", "linear_ln_mid"], ["set_option", "linear_ln_mid", engines.MID_GEMM_ROWS]]
    assert calls[-2][0] == "set_option" and calls[-2][2] == ["linear_ln_mid", 1] and calls[-1][0] == "wrapper_head"
    assert sum(_is_ln_option(c) for c in calls) == 3
    # every other line is the unflagged engine's; each linear_ln is the pair it replaces
    rest = [c for c in calls if not _is_ln_option(c)]
    assert etl.expand(rest, D) == want
    assert len(want) - len(rest) == 2 * full


@pytest.mark.parametrize("name", list(etl.UNCHANGED))
def test_flag_unset_or_ignored_records_the_golden_case(base, name):
    model, kw, env, base_case = etl.UNCHANGED[name]
    assert etl.record(model, kw, env) == base[base_case]


def test_explicit_flag_is_refused_with_fused_ln_and_mxfp8():
    import yvhip
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        engine_trace._patch(mp, rec)
        for kw in (dict(fused_ln=True, ln_gemm=True), dict(dtype="mxfp8", ln_gemm=True)):
            with pytest.raises(yvhip.YvError, match="ln_gemm"):
                etl.build(mp, engine_trace.P16, kw, {})
        assert etl.build(mp, engine_trace.P16, dict(ln_gemm=True, mid_gemm=True, long_attn=True), {}).ln_gemm
