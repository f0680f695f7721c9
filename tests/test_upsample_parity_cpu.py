"""The upsampler convolutions as four 2x2 sub-pixel convolutions (packing.up4_weights / pack_up4): the algebra against
conv2d(interpolate(x, 2, "nearest"), w, b, padding=1) in fp64, and the packed layout against the K order of gemm_pp.hip AMODE 4."""
import pytest
import torch
import torch.nn.functional as F

from mvd_amd.packing import pack_up4, up4_weights


def up4_reference(x, w4, bias):
    """What the kernel computes, written out: parity (py, px) of the output is a 2x2 convolution of the source map whose window
    starts at (i + py - 1, j + px - 1), taps outside the map being zero.  x (B, C, H, W), w4 (4, Cout, Cin, 2, 2)."""
    b, _, h, w = x.shape
    out = x.new_zeros(b, w4.shape[1], 2 * h, 2 * w)
    for py in (0, 1):
        for px in (0, 1):
            # window rows i+py-1, i+py: pad one row on top for py = 0, one at the bottom for py = 1 (same along x)
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            out[:, :, py::2, px::2] = F.conv2d(xp, w4[py * 2 + px])
    return out + bias[None, :, None, None]


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (8, 12), (2, 9)])
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_subpixel_form_equals_conv_of_upsampled_map_fp64(h, w, batch):
    g = torch.Generator().manual_seed(100 * h + 10 * w + batch)
    cin, cout = 6, 5
    x = torch.randn(batch, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, bias, padding=1)
    w4 = up4_weights(wt)
    assert w4.dtype == torch.float64 and tuple(w4.shape) == (4, cout, cin, 2, 2)
    got = up4_reference(x, w4, bias)
    err = (got - want).abs().max().item()
    print(f"sub-pixel form vs conv(interpolate) {batch}x{h}x{w}: max |difference| {err:.3g}")
    assert err <= 1e-12, err


def test_pack_up4_layout_matches_the_kernels_k_order():
    """Parity p, tap t = ty*2+tx, channel c of output channel n sits at [p][n][(c // 64) * 256 + t * 64 + c % 64]; the value is the
    fp32 sum rounded to bf16 once."""
    g = torch.Generator().manual_seed(7)
    cin, cout = 128, 3
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    packed = pack_up4(wt)
    assert packed.dtype == torch.bfloat16 and tuple(packed.shape) == (4, cout, 4 * cin) and packed.is_contiguous()
    w4 = up4_weights(wt)                                   # fp32 sums
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}            # parity -> 3x3 rows (columns) summed into tap 0 / tap 1
    for p in range(4):
        py, px = p >> 1, p & 1
        for t in range(4):
            ty, tx = t >> 1, t & 1
            for c in (0, 1, 63, 64, 127):
                for n in range(cout):
                    s = sum(wt[n, c, ky, kx] for ky in rows[py][ty] for kx in rows[px][tx])
                    assert torch.equal(w4[p, n, c, ty, tx], s) or abs(w4[p, n, c, ty, tx] - s) <= 1e-6
                    want = w4[p, n, c, ty, tx].to(torch.bfloat16)
                    assert packed[p, n, (c // 64) * 256 + t * 64 + c % 64] == want, (p, t, c, n)


def test_pack_up4_rejects_channel_counts_the_kernel_cannot_slice():
    with pytest.raises(AssertionError):
        pack_up4(torch.zeros(4, 48, 3, 3))


def test_pack_unet_registers_the_twin_in_lean_packing_too():
    """``up_blocks.{i}.up.w4`` next to ``.up.w`` wherever Cin % 64 == 0, with or without the small-batch twins (cfg4 runs lean)."""
    from mvd_amd.config import UNetConfig
    from mvd_amd.packing import pack_unet
    from oracle import sd21_unet as OU                     # (test infrastructure: seeded weights of the tiny topology)
    cfg = UNetConfig.tiny()
    sd = OU.init_params(OU.UNetConfig.tiny(), seed=3)
    seen = 0
    for lean in (False, True):
        packed = pack_unet(sd, cfg, "cpu", adapter=False, small_batch_twins=not lean)
        for i in range(cfg.num_levels - 1):
            wu = sd[f"up_blocks.{i}.upsamplers.0.conv.weight"]
            key = f"up_blocks.{i}.up.w4"
            assert f"up_blocks.{i}.up.w" in packed
            assert (key in packed) == (wu.shape[1] % 64 == 0), key
            if key in packed:
                assert torch.equal(packed[key], pack_up4(wu)) and packed[key].numel() == 16 * wu.shape[0] * wu.shape[1]
                seen += 1
    assert seen > 0
