"""The bits that yv_attention, yv_attention_train, yv_attention_mxfp8 and yv_attention_long write, against
tests/golden/attn_fwd_bits.json (attn_fwd_bits.py: cases, inputs, hashing, recorder).  The three kernel families behind them share one
text of their arithmetic and addresses (csrc/attention_fwd_core.h), so the tests that compare them with each other cannot see a change
of it; this one compares each with what it wrote before the text was shared."""
import pytest

import attn_fwd_bits as bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module")
def fixture():
    return bits.load_fixture()


@pytest.mark.parametrize("form,debug,R,N,H", bits.CASES)
def test_attention_fwd_recorded_bits(yv, fixture, form, debug, R, N, H):
    want = fixture[bits.case_id(form, debug, R, N, H)]
    got = bits.run_case(yv, form, debug, R, N, H)
    assert got["bits"] == want["bits"], "the bits written changed"
    assert got["tail_kept"], "something past the live rows of an output buffer was written"
