"""Bit-exact cases of the FreeU operator (``mvd_op_freeu``): answers that have ONE bit pattern, so that a
dropped pixel, a channel or an image booked to its neighbour, a lost 1 / (H W) or a second rounding is a mismatch, not an error
inside a tolerance.

* the backbone half: ``(x.float() * b).bfloat16()`` below C // 2 and the input's bits above, b in {1.4, 1.6, 1.0};
* s = 1: the skip map comes back bit for bit (-0.0 included);
* maps of 2 x 2, 2 x 4 and 4 x 4: every twiddle is 0 or +-1 (the kernel builds its table with the angle in half turns), and with
  s - 1 a power of two (s = 0.5, s = 2) an impulse map of small integers has an integer answer below 256, which bf16 holds
  exactly: whatever the order of the fp32 sums, there is one right bit pattern.  Channel c of image i carries one impulse at
  pixel (c + 5 i) mod H W, of value +-32 (1 + (c + i) mod 3): every pixel is the hot one in some channel, every channel in every
  image, and neighbours in either direction differ in place and value."""
import pytest
import torch

from tests import freeu_ref as FR

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("b", [1.4, 1.6, 1.0])
@pytest.mark.parametrize("C", [64, 24, 1280])
def test_backbone_half_is_one_rounding(C, b):
    _gpu()
    from mvd_amd import ops
    g = torch.Generator().manual_seed(C)
    hidden = (torch.randn(3, 36, C, generator=g) * 3).bfloat16()
    hidden[0, 0, 0], hidden[1, 5, C - 1] = -0.0, -0.0
    skip = torch.randn(3, 36, 8, generator=g).bfloat16()
    got, _ = ops.freeu(hidden.cuda(), skip.cuda(), 6, 6, b, 0.9)
    got = got.cpu()
    half = C // 2
    assert torch.equal(got[..., :half].view(torch.int16), (hidden[..., :half].float() * b).bfloat16().view(torch.int16))
    assert torch.equal(got[..., half:].view(torch.int16), hidden[..., half:].view(torch.int16))


@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (8, 8), (12, 12)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_s_one_returns_the_skip_bit_for_bit(hw):
    _gpu()
    from mvd_amd import ops
    H, W = hw
    g = torch.Generator().manual_seed(H * W)
    skip = torch.randn(2, H * W, 72, generator=g).bfloat16()
    skip[0, 0, 0], skip[1, H * W - 1, 71] = -0.0, -0.0
    hidden = torch.randn(2, H * W, 8, generator=g).bfloat16()
    _, got = ops.freeu(hidden.cuda(), skip.cuda(), H, W, 1.4, 1.0)
    assert torch.equal(got.cpu().view(torch.int16), skip.view(torch.int16))


def impulse_maps(B, H, W, C):
    """(B, C, H, W) fp32: channel c of image i holds +-32 (1 + (c + i) mod 3) at pixel (c + 5 i) mod H W, zero elsewhere"""
    x = torch.zeros(B, C, H * W)
    for i in range(B):
        c = torch.arange(C)
        v = 32.0 * (1 + (c + i) % 3) * torch.where((c // 3) % 2 == 0, 1.0, -1.0)
        x[i, c, (c + 5 * i) % (H * W)] = v
    return x.reshape(B, C, H, W)


@pytest.mark.parametrize("s", [0.5, 2.0])
@pytest.mark.parametrize("Cs", [72, 640])
@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 2), (4, 4)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_impulse_maps_have_one_answer(hw, Cs, s):
    _gpu()
    from mvd_amd import ops
    H, W = hw
    B = 3
    x = impulse_maps(B, H, W, Cs)
    want64 = FR.closed_form(x, s)
    want = want64.round()
    assert (want64 - want).abs().max().item() < 1e-9 and want.abs().max().item() < 256        # integers that bf16 holds exactly
    assert torch.equal(want.float().bfloat16().double(), want)
    assert len({int((c + 5 * i) % (H * W)) for c in range(Cs) for i in range(1)}) == H * W     # every pixel is hot somewhere
    hidden = torch.zeros(B, H * W, 8).bfloat16()
    _, got = ops.freeu(hidden.cuda(), FR.nhwc(x).bfloat16().cuda(), H, W, 1.0, s)
    got = FR.nchw(got.cpu().double(), H, W)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} mismatches, first (image, channel, h, w) = {bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {want[tuple(bad[0])].item()}"
