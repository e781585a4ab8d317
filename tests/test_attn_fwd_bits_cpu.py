"""tests/golden/attn_fwd_bits.json holds exactly the cases of attn_fwd_bits.py: a case dropped from the fixture, or a field dropped
from a case, must not pass silently (test_gpu_attn_fwd_bits.py looks up only what it runs)."""
import re

import attn_fwd_bits as bits


def test_case_ids_are_distinct():
    ids = [bits.case_id(*c) for c in bits.CASES]
    assert len(set(ids)) == len(ids)


def test_fixture_holds_exactly_the_cases():
    fixture = bits.load_fixture()
    assert list(fixture) == [bits.case_id(*c) for c in bits.CASES]
    for cid, val in fixture.items():
        assert tuple(val) == bits.FIELDS, cid
        assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in val.values()), cid


def test_cases_cover_every_instance_edge():
    """Both edges (32 NT - 31 and 32 NT) of every single-tile instance on the default and the one-item route, and the lengths at
    which the long kernel's launch plan changes."""
    by = lambda form, debug: {c[3] for c in bits.CASES if c[0] == form and c[1] == debug and c[2:] != (1, 197, 3)}
    for nt in range(1, 8):
        for form in bits.DEFAULT_FORMS:
            assert {32 * nt - 31, 32 * nt} <= by(form, 0), (form, nt)
        assert {32 * nt - 31, 32 * nt} <= by("attention", 5), nt
    for form in bits.DEFAULT_FORMS:
        assert {197, 225, 256, 257, 512, 513, 785} <= by(form, 0), form
    assert by("attention", 4) == {33, 197}
    for form in bits.LONG_FORMS:
        assert by(form, 0) == {1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 577, 785}, form
    assert ("attention", 0, 1, 197, 3) in bits.CASES and ("attention_train", 0, 1, 197, 3) in bits.CASES
