"""The path-pinned EfficientNMS cases (tests/nms_cases.py) reach the device paths they are there for, by the CPU path model and
oracle/boxes.py alone - no GPU."""
import pytest
import torch

import nms_cases as nc_


@pytest.mark.parametrize("name", sorted(nc_.CASES))
def test_case_reaches_its_paths(name):
    want = nc_.CASES[name][2]
    assert want <= set(nc_.PATHS)
    got = nc_.case_paths(name)
    assert want <= got, (name, sorted(want - got))


def test_every_modelled_path_is_reached():
    reached = set()
    for name in nc_.CASES:
        reached |= nc_.case_paths(name)
    assert reached <= set(nc_.PATHS)
    assert reached == set(nc_.PATHS), sorted(set(nc_.PATHS) - reached)


def test_model_claims_general_only_where_certain():
    # an image the head takes whole (fewer candidates than it holds) and one whose scan may or may not end inside the head's
    # window (sparse boxes: max_out are kept): neither is `general`
    boxes, scores = nc_.clustered(1, 300, 2, 4, seed=0)
    assert "general" not in nc_.paths(boxes, scores, thr=0.5)
    g = torch.Generator().manual_seed(0)
    xy = torch.rand(1, 4000, 2, generator=g) * 600
    boxes = torch.cat([xy, xy + 8], -1).contiguous()
    scores = torch.rand(1, 4000, 1, generator=g)
    got = nc_.paths(boxes, scores)
    assert "general" not in got and "heavy" not in got and got >= {"head16", "seg_list", "tail", "filter_tail_chunk"}


def test_list_capacity_matches_the_launcher_rule():
    assert nc_.list_capacity(8400, 5, 4096) == 45056 and nc_.list_capacity(4000, 12, 4096) == 45056
    assert nc_.list_capacity(501, 5, 4096) == 4096 and nc_.list_capacity(501, 5, 100) == 4096
    assert nc_.list_capacity(10, 1, 100) == 4096 and nc_.list_capacity(2500, 4, 4096) == 12288
