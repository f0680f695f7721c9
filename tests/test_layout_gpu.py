"""The launch schedule of every batch layout -- plain, views, objects, ragged -- is the one recorded before the layouts became one
value (tests/golden/layout_launch_tables.json, written by tools/record_layout_launch_tables.py at that commit): the same kernel
classes at the same shapes, as often, in the same order of first appearance.  Equal tables, no tolerance: a difference means the
schedule changed, and the thing to do is to find out why, not to record again."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "layout_launch_tables.json")


@pytest.fixture(scope="module")
def tables():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_layout_launch_tables as rec
    finally:
        sys.path.pop(0)
    return rec.record()


@pytest.mark.parametrize("name", ["plain", "views", "objects", "ragged_3_2_1", "ragged_2_2", "objects_2x2_g1"])
def test_launch_table_is_the_recorded_one(tables, name):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = tables[name]
    diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want[name])) if a != b]
    assert len(got) == len(want[name]) and not diff, (len(got), len(want[name]), diff[:5])


def test_equal_counts_launch_what_the_objects_forward_launches(tables):
    assert tables["ragged_2_2"] == tables["objects_2x2_g1"]
