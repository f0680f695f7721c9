"""The FreeU operator (``mvd_op_freeu``) on the MI355X against the fp64 closed form of tests/freeu_ref.py.

Tolerance: the project's operator convention -- max|err| of the skip output is at most ONE bf16 ulp of the largest output (the
kernel rounds once, half an ulp of the element at most; its fp32 sums and twiddles add ~1e-6 relative).  The backbone half is
exact: ``(x.float() * b).bfloat16()`` below C // 2, the input's bits above.

Shapes: the smallest that cross every boundary of the kernel's partition -- a workgroup is 8 channel octets x 32 pixel lanes and
owns 64 skip channels of one image: maps of 4, 8, 9 pixels (fewer than the pixel lanes), 32 (exactly), 36, 64, 144, 256 (several
walks); 8 skip channels (one octet of one chunk), 72 (a full chunk and one octet), 128, 640; 24 hidden channels put C // 2 inside
an octet; one large case makes the backbone workgroups walk their grid-stride loop a second time."""
import math

import pytest
import torch

from tests import freeu_ref as FR

pytestmark = pytest.mark.gpu

MAPS = [(2, 2), (2, 4), (3, 3), (4, 8), (6, 6), (8, 8), (12, 12), (16, 16)]
CHANNELS = [(128, 128), (1280, 640), (64, 8), (24, 72)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _inputs(B, H, W, C, Cs, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * B + 131 * H + 17 * W + C + 3 * Cs)
    hidden = torch.randn(B, H * W, C, generator=g).bfloat16()
    skip = torch.randn(B, H * W, Cs, generator=g).bfloat16()
    return hidden, skip


def bf16_ulp_of(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 7)


def _check(B, H, W, C, Cs, b, s):
    from mvd_amd import ops
    hidden, skip = _inputs(B, H, W, C, Cs)
    got_h, got_s = ops.freeu(hidden.cuda(), skip.cuda(), H, W, b, s)
    torch.cuda.synchronize()
    got_h, got_s = got_h.cpu(), got_s.cpu()
    want_s = FR.nhwc(FR.closed_form(FR.nchw(skip.float(), H, W), s))
    err = (got_s.double() - want_s).abs().max().item()
    ulp = bf16_ulp_of(want_s.abs().max().item())
    print(f"freeu B={B} {H}x{W} C={C} Cs={Cs} b={b} s={s}: max|err| {err:.4g}, one bf16 ulp of the largest output {ulp:.4g}")
    assert err <= ulp
    half = C // 2
    assert torch.equal(got_h[..., :half], (hidden[..., :half].float() * b).bfloat16())
    assert torch.equal(got_h[..., half:], hidden[..., half:])
    return got_s


@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: f"C{c[0]}-Cs{c[1]}")
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("B", [1, 3])
def test_freeu_against_the_closed_form(B, hw, channels):
    _gpu()
    for b, s in ((1.4, 0.9), (1.6, 0.2)):
        _check(B, *hw, *channels, b, s)


def test_freeu_backbone_grid_stride():
    """3 x 32 x 32 x 1536: more 16-byte vectors than one pass of the backbone workgroups holds"""
    _gpu()
    _check(3, 32, 32, 1536, 64, 1.6, 0.2)


def test_freeu_wrong_variants_are_outside_the_tolerance():
    """the tolerance above tells the flipped (1, 1) mode and the missing DC mode from the right function at the SD-2.1 strength"""
    _gpu()
    H, W = 8, 8
    got = _check(1, H, W, 128, 128, 1.6, 0.2)
    _, skip = _inputs(1, H, W, 128, 128)
    x = FR.nchw(skip.float(), H, W)
    ulp = bf16_ulp_of(FR.closed_form(x, 0.2).abs().max().item())
    for kw in (dict(flip_one_axis=True), dict(drop_dc=True)):
        assert (got.double() - FR.nhwc(FR.closed_form(x, 0.2, **kw))).abs().max().item() > 4 * ulp


def test_freeu_is_deterministic():
    """two launches on the same input: the same bits (fixed-order sums, no atomics)"""
    _gpu()
    from mvd_amd import ops
    for (H, W), (C, Cs), B in (((16, 16), (1280, 640), 3), ((12, 12), (128, 128), 1), ((3, 3), (24, 72), 3)):
        hidden, skip = (t.cuda() for t in _inputs(B, H, W, C, Cs, seed=5))
        h1, s1 = ops.freeu(hidden, skip, H, W, 1.4, 0.2)
        h2, s2 = ops.freeu(hidden, skip, H, W, 1.4, 0.2)
        torch.cuda.synchronize()
        assert torch.equal(h1, h2) and torch.equal(s1, s2)


def test_freeu_refusals():
    """H = 1, C % 8 != 0, s <= 0 and aliased outputs each raise, and nothing is launched: the outputs keep their fill"""
    _gpu()
    from mvd_amd import _lib as L
    from mvd_amd import ops
    fill = 7.0

    def outs(h, s):
        return torch.full_like(h, fill), torch.full_like(s, fill)

    def refused(match, hidden, skip, H, W, b, s, ho=None, so=None):
        keep = ho is None
        if keep:
            ho, so = outs(hidden, skip)
        with pytest.raises(L.MvdError, match=match):
            ops.freeu(hidden, skip, H, W, b, s, hidden_out=ho, skip_out=so)
        torch.cuda.synchronize()
        if keep:
            assert bool((ho == fill).all()) and bool((so == fill).all())

    hidden, skip = (t.cuda() for t in _inputs(2, 4, 4, 64, 64))
    row_h, row_s = (t.cuda() for t in _inputs(2, 1, 16, 64, 64))
    refused("at least 2 x 2", row_h, row_s, 1, 16, 1.4, 0.2)
    refused("at least 2 x 2", row_h, row_s, 16, 1, 1.4, 0.2)
    odd_h, odd_s = (t.cuda() for t in _inputs(2, 4, 4, 12, 64))
    refused("multiples of 8", odd_h, odd_s, 4, 4, 1.4, 0.2)
    odd_h, odd_s = (t.cuda() for t in _inputs(2, 4, 4, 64, 20))
    refused("multiples of 8", odd_h, odd_s, 4, 4, 1.4, 0.2)
    for b, s in ((1.4, 0.0), (1.4, -0.2), (0.0, 0.2), (float("nan"), 0.2), (1.4, float("inf"))):
        refused("positive and finite", hidden, skip, 4, 4, b, s)
    before_h, before_s = hidden.clone(), skip.clone()
    refused("overlaps", hidden, skip, 4, 4, 1.4, 0.2, ho=hidden, so=torch.empty_like(skip))
    refused("overlaps", hidden, skip, 4, 4, 1.4, 0.2, ho=torch.empty_like(hidden), so=skip)
    refused("overlaps", hidden, skip, 4, 4, 1.4, 0.2, ho=skip, so=torch.empty_like(skip))       # (same size here: C == Cs)
    both = torch.empty(2 * hidden.numel(), device="cuda", dtype=torch.bfloat16)
    refused("overlaps", hidden, skip, 4, 4, 1.4, 0.2, ho=both[:hidden.numel()].view_as(hidden), so=both[8:8 + skip.numel()].view_as(skip))
    torch.cuda.synchronize()
    assert torch.equal(hidden, before_h) and torch.equal(skip, before_s)
    with pytest.raises(L.MvdError, match="expected hidden"):
        ops.freeu(hidden, skip, 4, 8, 1.4, 0.2)
