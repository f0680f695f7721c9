"""SSIM / MSE / PSNR restated from their definitions (the SSIM of pytorch_msssim 1.0.0's defaults, torchmetrics' PSNR), in
fp64 by default: the reference of tests/test_validation_gpu.py.  ``dtype=torch.float32`` evaluates the same algorithm in
the precision the library itself uses; its drift against fp64 is the basis of the GPU bound (tests/test_validation_cpu.py).

    window = exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1, applied along H then W without padding
    mu = filt(x) ; sigma^2 = filt(x^2) - mu^2 ; sigma_12 = filt(x y) - mu_1 mu_2 ; C1 = (0.01 R)^2 ; C2 = (0.03 R)^2
    map = (2 mu_1 mu_2 + C1) / (mu_1^2 + mu_2^2 + C1) * (2 sigma_12 + C2) / (sigma_1^2 + sigma_2^2 + C2)
    ssim = mean over (image, channel) of the map's mean
"""
import math

import torch
import torch.nn.functional as F

WIN_SIZE, WIN_SIGMA = 11, 1.5


def gaussian_window(dtype=torch.float64):
    c = torch.arange(WIN_SIZE, dtype=dtype) - WIN_SIZE // 2
    g = torch.exp(-(c ** 2) / (2 * WIN_SIGMA ** 2))
    return g / g.sum()


def _filt(x, win):
    ch = x.shape[1]
    x = F.conv2d(x, win.view(1, 1, -1, 1).repeat(ch, 1, 1, 1), groups=ch)
    return F.conv2d(x, win.view(1, 1, 1, -1).repeat(ch, 1, 1, 1), groups=ch)


def ssim_per_channel(x, y, data_range, dtype=torch.float64):
    """(N, C, H, W) x 2 -> (N, C)"""
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    assert x.shape == y.shape and x.dim() == 4 and min(x.shape[2:]) >= WIN_SIZE
    win = gaussian_window(dtype)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = _filt(x, win), _filt(y, win)
    s11 = _filt(x * x, win) - mu1 * mu1
    s22 = _filt(y * y, win) - mu2 * mu2
    s12 = _filt(x * y, win) - mu1 * mu2
    m = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * ((2 * s12 + c2) / (s11 + s22 + c2))
    return m.flatten(2).mean(-1)


def ssim(x, y, data_range, dtype=torch.float64):
    return ssim_per_channel(x, y, data_range, dtype).mean()


def ssim_per_image(x, y, data_range, dtype=torch.float64):
    return ssim_per_channel(x, y, data_range, dtype).mean(1)


def mse(x, y):
    return ((x.detach().cpu().double() - y.detach().cpu().double()) ** 2).mean()


def mse_per_image(x, y):
    return ((x.detach().cpu().double() - y.detach().cpu().double()) ** 2).flatten(1).mean(1)


def psnr(x, y, data_range):
    m = float(mse(x, y))
    return math.inf if m == 0.0 else 10.0 * math.log10(data_range ** 2 / m)


def smooth_image(n, c, h, w, seed):
    """A low-frequency image in about [-0.8, 0.8]: a few sinusoids per channel."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, h).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w).view(1, 1, 1, w)
    img = torch.zeros(n, c, h, w)
    for _ in range(4):
        fy, fx, ph = (torch.rand(n, c, 1, 1, generator=g) * s for s in (6.0, 6.0, 6.28))
        img = img + 0.2 * torch.sin(fy * yy * 6.28 + fx * xx * 6.28 + ph)
    return img


def cases():
    """name -> (x, y, data_range, kind): the seven inputs of the drift record and the GPU bound ("natural": |SSIM error|
    <= 5e-6, "flat": <= 2e-4, "identical": |1 - SSIM| <= 1e-6), then further shapes held to the natural bound."""
    g = torch.Generator().manual_seed(1234)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    out = {}
    out["uniform_noise_4x3x64x64"] = (torch.rand(4, 3, 64, 64, generator=g) * 2 - 1, torch.rand(4, 3, 64, 64, generator=g) * 2 - 1,
                                      2.0, "natural")
    s = smooth_image(4, 3, 64, 64, 1)
    out["smooth_noise0.05_4x3x64x64"] = (s, s + 0.05 * rn(4, 3, 64, 64), 2.0, "natural")
    s = smooth_image(1, 3, 512, 512, 2)
    out["smooth_noise0.1_1x3x512x512"] = (s, s + 0.1 * rn(1, 3, 512, 512), 2.0, "natural")
    s = smooth_image(2, 3, 40, 72, 3)
    out["smooth_noise0.02_2x3x40x72"] = (s, s + 0.02 * rn(2, 3, 40, 72), 2.0, "natural")
    out["flat0.999_noise1e-3_2x3x32x32"] = (0.999 + 1e-3 * rn(2, 3, 32, 32), 0.999 + 1e-3 * rn(2, 3, 32, 32), 2.0, "flat")
    out["const0.4_vs_-0.7_1x1x11x11"] = (torch.full((1, 1, 11, 11), 0.4), torch.full((1, 1, 11, 11), -0.7), 2.0, "flat")
    s = smooth_image(2, 3, 48, 48, 4) + 0.1 * rn(2, 3, 48, 48)
    out["identical_2x3x48x48"] = (s, s.clone(), 2.0, "identical")
    return out


def extra_shape_cases():
    g = torch.Generator().manual_seed(4321)
    out = {}
    s = smooth_image(3, 1, 12, 75, 5)
    out["one_channel_3x1x12x75"] = (s, s + 0.05 * torch.randn(3, 1, 12, 75, generator=g), 2.0, "natural")
    s = smooth_image(1, 3, 768, 768, 6)
    out["smooth_noise0.05_1x3x768x768"] = (s, s + 0.05 * torch.randn(1, 3, 768, 768, generator=g), 2.0, "natural")
    s = smooth_image(2, 5, 27, 139, 7)
    out["five_channels_2x5x27x139"] = (s, s + 0.05 * torch.randn(2, 5, 27, 139, generator=g), 1.0, "natural")
    return out
