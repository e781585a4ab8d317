"""The bits that yv_attention_bwd, yv_attention_bwd_long and yv_attention_bwd_short write, against tests/golden/attn_bwd_bits.json
(attn_bwd_bits.py: cases, inputs, hashing, recorder).  The three entry points share one text of their arithmetic
(csrc/attention_bwd_core.h), so the tests that compare them with each other cannot see a change of it; this one compares each with
what it wrote before the text was shared."""
import pytest

import attn_bwd_bits as bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module")
def fixture():
    return bits.load_fixture()


@pytest.mark.parametrize("kernel,R,N,H", bits.CASES)
def test_attention_bwd_recorded_bits(yv, fixture, kernel, R, N, H):
    want = fixture[bits.case_id(kernel, R, N, H)]
    got = bits.run_case(yv, kernel, R, N, H)
    assert got["operands"] == want["operands"], \
        "out / lse differ from the recording: the inputs or the forward (yv_attention_train) changed, not the backward"
    assert got["dqkv"] == want["dqkv"], "dqkv bits changed"
    assert got["delta"] == want["delta"], "delta_ws bits changed"
    assert got["tail_kept"], "rows past R*N of dqkv or floats past R*H*N of delta_ws were written"
