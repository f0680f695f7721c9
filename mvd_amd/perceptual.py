"""VGG-16 perceptual loss on the MI355X: ``PerceptualLoss`` of the reference's
src/training/losses.py:21-56 -- torchvision's ``vgg16(...).features[:29]`` on both image batches and ``F.mse_loss`` of the two
conv5_3 maps -- without torchvision, on the HIP kernels of libmvd_hip.so (``mvd_vgg_*``, csrc/vgg.hip).

* ``VGG16FeaturesHIP`` -- an ``nn.Module`` whose parameters carry torchvision's key names (``features.0.weight`` ...
  ``features.28.bias``), so ``vgg16-397923af.pth`` loads with ``load_state_dict``.  It has no torch forward: ``forward`` hands
  device pointers to ``mvd_vgg_features``.
* ``PerceptualLoss`` -- the reference's constructor, ``__call__(x, y)`` and ``.to(device)``, plus ``per_sample(x, y)`` (val.py
  calls the loss once per sample for that).  One ``mvd_vgg_perceptual`` call; the result is a 0-d device tensor, nothing
  synchronises.

Nothing is ever fetched: weights come from a path, a state dict, or the local torch hub cache.  CPU tensors raise ``MvdError``:
there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Union

import torch
from torch import nn

from . import _lib as L
from .hub import hub_checkpoint_dirs, resolve_state_dict      # (hub_checkpoint_dirs stays importable from here)
from .packing import VGG16_CONVS, normalize_vgg_keys, pack_vgg

VGG16_FILE = "vgg16-397923af.pth"          # torchvision's VGG16_Weights.IMAGENET1K_V1
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3")
TAP_CHANNELS = (64, 128, 256, 512)


def load_vgg16_weights(weights: Union[None, str, os.PathLike, Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """A state dict from ``weights``: a dict as it is, a ``.pth`` / ``.safetensors`` path, or ``None`` = ``vgg16-397923af.pth`` in the
    local hub cache.  Never downloads: a file that is not there raises ``MvdError``."""
    tried = [os.path.join(d, VGG16_FILE) for d in hub_checkpoint_dirs()]
    if weights is None and not any(os.path.isfile(p) for p in tried):      # (this module's own wording of "no file found")
        raise L.MvdError(f"PerceptualLoss: {VGG16_FILE} not found in {tried} and nothing is downloaded: put torchvision's "
                         "VGG-16 checkpoint there, or pass weights=<path or state dict>")
    return resolve_state_dict(weights, tried, "PerceptualLoss", "weights")


class _Conv(nn.Module):
    """Parameter holder of one 3x3 convolution (no initialisation: the values come from ``load_state_dict``)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout), requires_grad=False)


class _VggHandle(L.Handle):
    """One ``mvd_vgg_t``; ``workspace(device, images, h, w)``."""

    def __init__(self):
        super().__init__("vgg")


def _images(t, who: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
        raise L.MvdError(f"{who}: images must be a (B, 3, H, W) tensor in [-1, 1], got {tuple(getattr(t, 'shape', ()))}")
    if not t.is_cuda:
        raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): got a tensor on {t.device}; there is no CPU fallback")
    if t.shape[2] < 16 or t.shape[3] < 16:
        raise L.MvdError(f"{who}: images of {t.shape[2]} x {t.shape[3]} are smaller than the tower's four pools need (16 x 16)")
    return t.detach().to(torch.float32).contiguous()


class VGG16FeaturesHIP(nn.Module):
    """torchvision's ``vgg16().features[:29]`` on the GPU kernels.  ``load_state_dict`` takes torchvision's keys
    (``features.N.*``; ``classifier.*`` is ignored) or those of the sliced ``Sequential`` (``N.*``)."""

    def __init__(self):
        super().__init__()
        self.features = nn.Module()
        for idx, cin, cout in VGG16_CONVS:
            self.features.add_module(str(idx), _Conv(cin, cout))
        self._loaded = False
        self._handle: Optional[_VggHandle] = None
        self._dev = None
        self._packed: Dict[str, torch.Tensor] = {}
        self._dirty = True

    def load_state_dict(self, sd, strict: bool = True, **kw):
        out = super().load_state_dict(normalize_vgg_keys(sd), strict=strict, **kw)
        self._loaded, self._dirty = True, True
        return out

    def to(self, *a, **k):
        self._dirty = True
        return super().to(*a, **k)

    def _sync(self, dev: torch.device):
        if not self._loaded:
            raise L.MvdError("VGG16FeaturesHIP has no weights: call load_state_dict first (nothing is downloaded)")
        if self._handle is None:
            self._handle = _VggHandle()
        if self._dirty or self._dev != dev:
            with torch.no_grad():
                self._packed = pack_vgg(self.state_dict(), dev)
            self._handle.set_weights(self._packed)
            self._dirty, self._dev = False, dev

    @torch.no_grad()
    def forward(self, images: torch.Tensor, taps: bool = False):
        """images (B, 3, H, W) in [-1, 1] (the normalisation is inside) -> the conv5_3 map (B, 512, H/16, W/16) fp32, an NCHW view
        of the NHWC buffer the kernels write.  ``taps=True``: also a dict of the four bf16 maps in front of the pools."""
        x = _images(images, "VGG16FeaturesHIP")
        self._sync(x.device)
        b, _, h, w = x.shape
        self._handle.workspace(x.device, b, h, w)
        feat = torch.empty(b, h // 16, w // 16, 512, device=x.device, dtype=torch.float32)
        tap_t, tap_p = [], None
        if taps:
            tap_t = [torch.empty(b, h >> i, w >> i, c, device=x.device, dtype=torch.bfloat16) for i, c in enumerate(TAP_CHANNELS)]
            tap_p = (C.c_void_p * 4)(*[t.data_ptr() for t in tap_t])
        L.call("mvd_vgg_features", self._handle.h, C.c_void_p(x.data_ptr()), b, h, w, C.c_void_p(feat.data_ptr()), tap_p, L.stream())
        out = feat.permute(0, 3, 1, 2)
        return (out, {n: t.permute(0, 3, 1, 2) for n, t in zip(TAP_NAMES, tap_t)}) if taps else out


class PerceptualLoss:
    """``PerceptualLoss(device)`` of the reference: ``loss(x, y)`` = mean squared difference of the conv5_3 maps of two image
    batches in [-1, 1].  ``weights``: a ``.pth`` / ``.safetensors`` path, a state dict, or ``None`` for ``vgg16-397923af.pth`` in
    the local torch hub cache.  ``max_pairs_per_pass`` caps the workspace: larger batches run in several passes of one call."""

    def __init__(self, device="cuda", weights=None, max_pairs_per_pass: int = 8):
        if int(max_pairs_per_pass) < 1:
            raise L.MvdError(f"PerceptualLoss: max_pairs_per_pass={max_pairs_per_pass!r} must be at least 1")
        self.vgg = VGG16FeaturesHIP()
        self.vgg.load_state_dict(load_vgg16_weights(weights))
        self.device = device
        self.max_pairs_per_pass = int(max_pairs_per_pass)

    def to(self, device):
        self.device = device
        return self

    def _run(self, x, y, per_pair: bool):
        x, y = _images(x, "PerceptualLoss"), _images(y, "PerceptualLoss")
        if x.shape != y.shape or x.device != y.device:
            raise L.MvdError(f"PerceptualLoss: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device} must match")
        if x.device != torch.device(self.device):      # the reference follows its input's device
            self.to(x.device)
        self.vgg._sync(x.device)
        b, _, h, w = x.shape
        hd = self.vgg._handle
        hd.workspace(x.device, 2 * min(b, self.max_pairs_per_pass), h, w)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        pp = torch.empty(b, device=x.device, dtype=torch.float32) if per_pair else None
        L.call("mvd_vgg_perceptual", hd.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), b, h, w, C.c_void_p(loss.data_ptr()),
               C.c_void_p(pp.data_ptr()) if per_pair else None, L.stream())
        return loss, pp

    @torch.no_grad()
    def __call__(self, x, y) -> torch.Tensor:
        return self._run(x, y, False)[0]

    @torch.no_grad()
    def per_sample(self, x, y) -> torch.Tensor:
        """(B,): the loss of every (x[b], y[b]) pair, what val.py:392-401 gets from one call per sample; their mean is ``loss(x, y)``."""
        return self._run(x, y, True)[1]
