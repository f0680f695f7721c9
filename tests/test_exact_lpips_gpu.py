"""Bit-exact tests of the kernels LPIPS adds in front of the GEMM tiles (csrc/lpips.hip): the 3x3 stride-2 max-pool, both im2col
forms, and the two AlexNet front-end convolutions end to end (im2col rows + packed weights + the ReLU GEMM, unsplit and through
the split-K reduce pass).

Everything is an integer (or a dyadic fraction) far below 2^24 and a bf16 value wherever it is stored, so the reference -- fp64 on
the CPU, ``F.unfold`` / ``F.max_pool2d`` / ``F.conv2d`` -- is exact and the comparison is ``torch.equal`` on the bit patterns.
Outputs sit in larger buffers of a sentinel value: nothing beyond them may be written."""
import pytest
import torch
import torch.nn.functional as F

import exact_util as X

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def guarded(n):
    return torch.full((n + GUARD,), -7.0, dtype=torch.bfloat16, device="cuda")


def check_guard(buf, n, what):
    assert torch.equal(buf[n:].cpu(), torch.full((GUARD,), -7.0, dtype=torch.bfloat16)), f"{what} wrote beyond its output"


# sizes 3 -> 1, 7 -> 3, 8 -> 3, 15 -> 7
@pytest.mark.parametrize("B,H,W", [(2, 3, 3), (1, 7, 8), (2, 15, 7)])
@pytest.mark.parametrize("c", [8, 64, 192])
def test_maxpool3x3s2_exact(ops, B, H, W, c):
    g = torch.Generator().manual_seed(B + 3 * H + 5 * W + c)
    x = (torch.randn(B, H, W, c, generator=g) * 4).to(torch.bfloat16)
    x[0, 0, 0, :8] = torch.tensor([0.0, 0.25, 1.0, -1.0, 3.0e38, -3.0e38, 2.0 ** -120, 0.5]).to(torch.bfloat16)
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    assert want.shape == (B, (H - 3) // 2 + 1, (W - 3) // 2 + 1, c)
    n = want.numel()
    buf = guarded(n)
    ops.maxpool3x3s2(x.cuda(), out=buf)
    X.assert_same_bits(buf[:n].reshape(want.shape), want, f"maxpool3x3s2 {(B, H, W, c)}")
    check_guard(buf, n, "maxpool3x3s2")
    X.assert_same_bits(ops.maxpool3x3s2(x.cuda()), want, "maxpool3x3s2 (own buffer)")


def unfold_rows(x_nchw, k, stride, pad):
    """F.unfold's (B, C k k, L) reordered to rows (B L, k k C) with column (ky k + kx) C + c"""
    B, Cn = x_nchw.shape[:2]
    u = F.unfold(x_nchw, k, padding=pad, stride=stride)
    return u.reshape(B, Cn, k, k, -1).permute(0, 4, 2, 3, 1).reshape(-1, k * k * Cn)


@pytest.mark.parametrize("B,H,W", [(2, 31, 38), (1, 47, 66), (3, 7, 9)])
@pytest.mark.parametrize("affine", [None, ((2.0, 0.5, 4.0), (1.0, -2.0, 0.5))], ids=["identity", "pow2"])
def test_im2col_patch_image_exact(ops, B, H, W, affine):
    g = torch.Generator().manual_seed(B + 3 * H + 5 * W)
    x = torch.randint(-7, 8, (B, 3, H, W), generator=g).double()
    scaled = x if affine is None else x * torch.tensor(affine[0]).double().view(1, 3, 1, 1) + torch.tensor(affine[1]).double().view(1, 3, 1, 1)
    # unfold pads the SCALED image with zeros: the border taps are zeros, not the shift
    rows = unfold_rows(scaled, 11, 4, 2)
    want = X.bf(F.pad(rows, (0, 384 - 363)))
    assert want.shape == (B * ((H - 7) // 4 + 1) * ((W - 7) // 4 + 1), 384)
    if affine is not None:
        assert (rows[0, :3 * 11 * 2] == 0).all() and rows[0, (2 * 11 + 2) * 3 + 2] != 0      # row 0: two rows of padding on top, then pixel (0, 0): 4 x + 0.5
    n = want.numel()
    buf = guarded(n)
    kw = {} if affine is None else dict(scale=affine[0], shift=affine[1])
    ops.im2col_patch(X.f32(x).cuda(), out=buf, **kw)
    got = buf[:n].reshape(want.shape)
    X.assert_same_bits(got, want, f"im2col_patch image {(B, H, W)} {affine}")
    assert torch.count_nonzero(got[:, 363:]) == 0
    check_guard(buf, n, "im2col_patch")


@pytest.mark.parametrize("B,H,W", [(2, 3, 3), (1, 5, 7), (3, 9, 4), (1, 1, 1)])
def test_im2col_patch_map_exact(ops, B, H, W):
    g = torch.Generator().manual_seed(7 + B + 3 * H + 5 * W)
    x = torch.randint(-100, 101, (B, H, W, 64), generator=g).double()
    want = X.bf(unfold_rows(x.permute(0, 3, 1, 2), 5, 1, 2))
    assert want.shape == (B * H * W, 1600)
    n = want.numel()
    buf = guarded(n)
    ops.im2col_patch(X.dev(x), out=buf)
    X.assert_same_bits(buf[:n].reshape(want.shape), want, f"im2col_patch map {(B, H, W)}")
    check_guard(buf, n, "im2col_patch")


def centred_bias(acc):
    return -acc.reshape(-1, acc.shape[-1]).median(0).values.round()


def conv_front_end(ops, x_dev, w, stride, pad, what):
    """im2col rows of x, the packed weights and the ReLU GEMM against F.conv2d in fp64 with ONE rounding; w ternary, the bias
    centred so that about half of the pre-ReLU outputs are negative"""
    from mvd_amd.packing import pack_alex_conv
    x64 = x_dev.double().cpu() if x_dev.dtype == torch.float32 else x_dev.double().cpu().permute(0, 3, 1, 2)
    acc = F.conv2d(x64, w, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    bias = centred_bias(acc)
    pre = acc + bias
    neg, pos = float((pre < 0).double().mean()), float((pre > 0).double().mean())
    assert neg >= 0.4 and pos >= 0.4, f"{what}: {neg:.1%} negative, {pos:.1%} positive pre-ReLU outputs"
    rows = ops.im2col_patch(x_dev)
    wp = X.dev(pack_alex_conv(w).double())
    assert rows.shape[1] == wp.shape[1]
    for splitk in (1, 4):
        for out_f32 in (False, True):
            got = ops.linear_relu(rows, wp, X.dev32(bias), relu=True, out_f32=out_f32, splitk=splitk)
            X.assert_same_bits(got.reshape(pre.shape), X.round_once(pre.clamp(min=0.0), out_f32), f"{what} split-K {splitk} fp32 {out_f32}")


def test_conv1_front_end_exact(ops):
    """11x11 stride 4 pad 2, 3 -> 64: |sum| <= 363 x 3, exact in fp32 in any order"""
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-3, 4, (2, 3, 31, 38), generator=g).double()
    w = torch.randint(-1, 2, (64, 3, 11, 11), generator=g).double()
    conv_front_end(ops, X.f32(x).cuda(), w, 4, 2, "conv1")


def test_conv2_front_end_exact(ops):
    """5x5 pad 2, 64 -> 192 (N = 192: the 64-column tiles): |sum| <= 1600 x 3"""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 5, 7, 64), generator=g).double()
    w = torch.randint(-1, 2, (192, 64, 5, 5), generator=g).double()
    conv_front_end(ops, X.dev(x), w, 1, 2, "conv2")
