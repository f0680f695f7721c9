"""References for FreeU, shared by tests/test_freeu_cpu.py and the three GPU test files.

(a) ``fourier_filter`` / ``apply_freeu``: diffusers 0.32.2 restated with ``torch.fft``;
(b) ``closed_form``: the rank-4 projection that the threshold-1 filter is, in fp64, with switches for the WRONG variants the
    tests must tell apart;
(c) ``freeu_oracle``: a context manager under which the oracle's forwards (``oracle.sd21_unet.unet_forward`` and everything
    built on it, ``oracle.mvd.multiview_unet_forward`` included) apply FreeU in the MAIN pass's up blocks.

Plain helper module, no fixtures; nothing here touches the code under test and ``oracle/`` is not edited: (c) swaps two module
attributes for the duration of the ``with`` block and puts them back."""
import contextlib
import math

import torch

from oracle import sd21_unet as OU

SD21 = dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6)       # the published SD-2.1 setting
# The setting of the engine parity tests.  Under the SD-2.1 setting the wrong functions (b only, s only, the flipped (1, 1) mode)
# sit 2e-2 .. 7e-2 from the right one on the tiny topology -- inside four times a parity bound of 2e-2 -- so the parity tests
# use values under which every one of them is at least 4 * PARITY_BOUND_MAX away (tests/test_freeu_cpu.py asserts it); distinct
# values per block, so that swapped blocks are a wrong function too.
PARITY_SETTING = dict(s1=16.0, s2=24.0, b1=2.0, b2=2.5)
# The engine parity bound is 1.5 x the rel-L2 of the SAME inputs with FreeU off against the plain oracle (amplified backbone
# channels amplify the bf16 error they carry), measured in the test itself, and never more than this:
PARITY_BOUND_MAX = 3e-2


# ---------------------------------------------------------------------------------------------- (a) diffusers, restated
def fourier_filter(x: torch.Tensor, threshold: int, scale: float) -> torch.Tensor:
    """diffusers.utils.torch_utils.fourier_filter: (B, C, H, W), computed in fp32, returned in x's dtype."""
    dtype = x.dtype
    x = x.to(torch.float32)
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    B, C, H, W = f.shape
    mask = torch.ones((B, C, H, W))
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    f = torch.fft.ifftshift(f * mask, dim=(-2, -1))
    return torch.fft.ifftn(f, dim=(-2, -1)).real.to(dtype)


def apply_freeu(resolution_idx: int, hidden: torch.Tensor, skip: torch.Tensor, s1, s2, b1, b2):
    """diffusers.utils.torch_utils.apply_freeu (functional: the inputs are not modified)."""
    if resolution_idx in (0, 1):
        b, s = (b1, s1) if resolution_idx == 0 else (b2, s2)
        half = hidden.shape[1] // 2
        hidden = hidden.clone()
        hidden[:, :half] = hidden[:, :half] * b
        skip = fourier_filter(skip, 1, s)
    return hidden, skip


# ---------------------------------------------------------------------------------------------- (b) the closed form
def closed_form(x: torch.Tensor, s: float, *, flip_one_axis: bool = False, drop_dc: bool = False) -> torch.Tensor:
    """skip' of (B, C, H, W) in fp64: x + (s - 1) / (H W) sum_kl (a_kl cos phi_kl + b_kl sin phi_kl), phi_kl = 2 pi (k h / H + l w / W),
    k, l in {0, 1}.  WRONG on purpose: ``flip_one_axis`` -- mode (1, 1) with phi = 2 pi (h / H - w / W); ``drop_dc`` -- mode (0, 0)
    left out."""
    x = x.to(torch.float64)
    H, W = x.shape[-2:]
    ph = 2.0 * math.pi * torch.arange(H, dtype=torch.float64)[:, None] / H
    pw = 2.0 * math.pi * torch.arange(W, dtype=torch.float64)[None, :] / W
    corr = torch.zeros_like(x)
    for k in (0, 1):
        for l in (0, 1):
            if drop_dc and k == 0 and l == 0:
                continue
            phi = k * ph + (-l if (flip_one_axis and k == 1 and l == 1) else l) * pw + torch.zeros(H, W, dtype=torch.float64)
            c, sn = torch.cos(phi), torch.sin(phi)
            a = (x * c).sum(dim=(-2, -1), keepdim=True)
            b = (x * sn).sum(dim=(-2, -1), keepdim=True)
            corr = corr + a * c + b * sn
    return x + (s - 1.0) / (H * W) * corr


def backbone_scale(hidden: torch.Tensor, b: float, *, upper_half: bool = False) -> torch.Tensor:
    """hidden (B, C, H, W) with channels [0, C // 2) times b.  WRONG on purpose: ``upper_half`` -- the other half."""
    half = hidden.shape[1] // 2
    out = hidden.clone()
    if upper_half:
        out[:, half:] = out[:, half:] * b
    else:
        out[:, :half] = out[:, :half] * b
    return out


def nhwc(x: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) -> token-major (B, H*W, C), contiguous: the engine's layout"""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()


def nchw(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    B, HW, C = x.shape
    return x.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------- (c) the FreeU oracle forward
@contextlib.contextmanager
def freeu_oracle(s1, s2, b1, b2, *, blocks=(0, 1), use_b=True, use_s=True, flip_one_axis=False):
    """Inside the block every MAIN-pass oracle forward applies FreeU in front of the resnets of up blocks ``blocks``: the
    concatenated input of ``up_blocks.{i}.resnets.{j}`` is split at the hidden channel count (the previous block's output for
    j = 0, else the block's own: ``oracle.sd21_unet.up_block_resnet_channels``), re-weighted and concatenated again.  The encoder
    pass (the one forward that passes ``capture``) runs without it, as the reference's ImageEncoder does; camera and adapter hooks
    are untouched.  Block 2 takes (b2, s2) when asked for (a WRONG variant; diffusers stops at block 1).  ``use_b`` / ``use_s``
    False and ``flip_one_axis``: the other wrong variants."""
    orig_forward, orig_resnet = OU.unet_forward, OU.resnet_block
    state = {"cfg": None}

    def forward(p, cfg, sample, timestep, text, attn_hook=None, block_hook=None, capture=None, **kw):
        prev = state["cfg"]
        state["cfg"] = cfg if capture is None else None
        try:
            return orig_forward(p, cfg, sample, timestep, text, attn_hook=attn_hook, block_hook=block_hook, capture=capture, **kw)
        finally:
            state["cfg"] = prev

    def resnet(p, key, x, temb_act, groups, eps):
        cfg = state["cfg"]
        if cfg is not None and key.startswith("up_blocks."):
            parts = key.split(".")
            i, j = int(parts[1]), int(parts[3])
            if i in blocks:
                hid = OU.up_block_resnet_channels(cfg)[i][j][0]
                b, s = (b1, s1) if i == 0 else (b2, s2)
                hidden, skip = x[:, :hid], x[:, hid:]
                if use_b:
                    hidden = backbone_scale(hidden, b)
                if use_s:
                    skip = closed_form(skip, s, flip_one_axis=True).to(x.dtype) if flip_one_axis else fourier_filter(skip, 1, s)
                x = torch.cat([hidden, skip], dim=1)
        return orig_resnet(p, key, x, temb_act, groups, eps)

    OU.unet_forward, OU.resnet_block = forward, resnet
    try:
        yield
    finally:
        OU.unet_forward, OU.resnet_block = orig_forward, orig_resnet
