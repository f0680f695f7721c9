"""The grouped reference normalisation (``ops.refnorm_grouped``: Q2 statistics over each run of ``group`` batch rows; group 1 is
the object forward's per-object form) against ``ops.refnorm`` on each slice of ``group`` rows, bit for
bit: the grouped kernel walks a group's elements in the ungrouped kernel's order for that many rows.  One object's rows are
8 x as large as the others', so a statistic booked to the neighbouring group (or taken over the whole batch) changes bits."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# B, group, hw, C: one workgroup pass and several per row (C / 8 against 256 threads), a group of every row, an odd pixel
# count with the smallest channel count, group == batch (the ungrouped kernel itself)
SHAPES = [(3, 1, 16, 64), (4, 2, 64, 320), (2, 1, 256, 1280), (6, 3, 5, 8), (5, 5, 16, 64)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def _features(B, group, hw, c):
    g = torch.Generator().manual_seed(1500 + B + 3 * group + 5 * hw + 7 * c)
    x = torch.randn(B, hw, c, generator=g) + 0.25
    x[(B // group - 1) * group:] *= 8.0            # the last group (object)
    return x.to(torch.bfloat16).cuda()


@pytest.mark.parametrize("B,group,hw,c", SHAPES)
def test_grouped_refnorm_is_refnorm_per_group(ops, B, group, hw, c):
    x = _features(B, group, hw, c)
    got = ops.refnorm_grouped(x, group)
    assert got.shape == x.shape and torch.isfinite(got.float()).all()
    for s in range(0, B, group):
        want = ops.refnorm(x[s:s + group].contiguous())
        assert torch.equal(got[s:s + group].view(torch.int16), want.view(torch.int16)), (s, group)
    if group < B:      # the scaled object makes the difference visible: whole-batch statistics give other bits in every group
        whole = ops.refnorm(x)
        for s in range(0, B, group):
            assert not torch.equal(got[s:s + group].view(torch.int16), whole[s:s + group].view(torch.int16)), s
    else:
        assert torch.equal(got.view(torch.int16), ops.refnorm(x).view(torch.int16))


def test_grouped_refnorm_rejects_bad_arguments(ops):
    from mvd_amd import _lib as L
    x = torch.zeros(4, 16, 64, dtype=torch.bfloat16, device="cuda")
    y = torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for group in (3, 0, -1, 8):
        assert L.lib().mvd_op_refnorm_grouped(p(x), 4, group, 16, 64, p(y), L.stream()) != 0
        assert "does not divide" in L.last_error(), (group, L.last_error())
    assert L.lib().mvd_op_refnorm_grouped(p(x), 4, 2, 16, 60, p(y), L.stream()) != 0      # c % 8
    assert "bad arguments" in L.last_error(), L.last_error()
    assert L.lib().mvd_op_refnorm_grouped(None, 4, 2, 16, 64, p(y), L.stream()) != 0
    assert "bad arguments" in L.last_error(), L.last_error()
