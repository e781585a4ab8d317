"""The bits that yv_wgrad_tiled, yv_wgrad_wide, yv_wgrad_conv3_tiled and yv_wgrad_conv3_gather write, against
tests/golden/wgrad_bits.json (wgrad_bits.py: cases, inputs, hashing, recorder).  The 128 x 128, narrow, wide and gather kernels are
instances of one text (gemm_tn_body in csrc/gemm.hip), so the tests that compare them with each other cannot see a change of it; this one compares
each with what it wrote while every tile shape had a text of its own."""
import pytest

import wgrad_bits as bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module")
def fixture():
    return bits.load_fixture()


@pytest.mark.parametrize("case", bits.CASES, ids=lambda c: bits.case_id(*c))
def test_wgrad_recorded_bits(yv, fixture, case):
    want = fixture[bits.case_id(*case)]
    got = bits.run_case(yv, *case)
    assert got["dw"] == want["dw"], "dW bits changed"
    assert got["tail_kept"], "something outside the dW window was written"
