"""LPIPS v0.1 on the MI355X: ``lpips.LPIPS(net="alex")`` of the reference's val.py:87 without the
``lpips`` package or torchvision, on the HIP kernels of libmvd_hip.so (``mvd_lpips_*``, csrc/lpips.hip).  The substitution is one
line: ``import mvd_amd.lpips as lpips``.

* ``net="alex"``: torchvision's ``alexnet().features[:12]`` (``ALEX_LAYERS`` below), five taps of 64, 192, 384, 256, 256
  channels; one ``mvd_lpips_distance`` call.
* ``net="vgg"``: a composition -- ``VGG16FeaturesHIP.forward(torch.cat([x, y]), taps=True)`` of perceptual.py (its front end is
  the same affine map: 2 mean - 1 and 2 std ARE the LPIPS shift and scale), then ``mvd_op_lpips_head`` over the four bf16 taps and
  the fp32 ``features.28`` map, whose ReLU the head applies.

Per tap: f^ = f / (sqrt(sum_c f^2) + 1e-10), d_l = mean_{h,w} sum_c w_c (f^x - f^y)^2; d = sum_l d_l.

Nothing is ever fetched: the backbone comes from ``backbone=`` (a state dict, a path, or torchvision's checkpoint in the local hub
cache), the linear heads from ``model_path=`` (a state dict, a path, the installed lpips package's ``weights/v0.1/<net>.pth`` -- found
without importing it -- or ``lpips-v0.1-<net>.pth`` in the hub cache).  CPU tensors raise ``MvdError``: there is no fallback.
What is not here: ``spatial=True``, ``net="squeeze"``, training of the heads (``lpips=False``, ``pnet_rand``, ``pnet_tune``), a
backward pass.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .hub import hub_checkpoint_dirs, resolve_state_dict
from .packing import (ALEX_CONVS, ALEX_TAP_CHANNELS, LPIPS_SCALE, LPIPS_SHIFT, VGG16_CONVS, VGG_LPIPS_TAP_CHANNELS, normalize_backbone_keys,
                      normalize_lpips_lin_keys, pack_alex)
from .perceptual import VGG16_FILE, TAP_NAMES, VGG16FeaturesHIP

ALEX_FILE = "alexnet-owt-7be5be79.pth"      # torchvision's AlexNet_Weights.IMAGENET1K_V1
# torchvision's alexnet().features[:12]
ALEX_LAYERS = (
    (0, "conv 3->64, 11x11, stride 4, pad 2"), (1, "relu"), (2, "max-pool 3x3, stride 2"),
    (3, "conv 64->192, 5x5, pad 2"), (4, "relu"), (5, "max-pool 3x3, stride 2"),
    (6, "conv 192->384, 3x3, pad 1"), (7, "relu"), (8, "conv 384->256, 3x3, pad 1"), (9, "relu"),
    (10, "conv 256->256, 3x3, pad 1"), (11, "relu"))
ALEX_TAPS = (1, 4, 7, 9, 11)                 # the ReLUs whose outputs the head compares
TAP_CHANNELS = {"alex": ALEX_TAP_CHANNELS, "vgg": VGG_LPIPS_TAP_CHANNELS}
MIN_SIZE = {"alex": 31, "vgg": 16}           # alex: below 31 the second pool has no output; vgg: four 2x2 pools
_BACKBONE_FILE = {"alex": ALEX_FILE, "vgg": VGG16_FILE}
_LPIPS_DEFAULTS = dict(pretrained=True, lpips=True, use_dropout=True, eval_mode=True, verbose=True, pnet_rand=False, pnet_tune=False)


def alex_tap_sizes(h: int, w: int) -> List[Tuple[int, int]]:
    """(h, w) of the five AlexNet taps of an h x w image"""
    c1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    p1 = ((c1[0] - 3) // 2 + 1, (c1[1] - 3) // 2 + 1)
    p2 = ((p1[0] - 3) // 2 + 1, (p1[1] - 3) // 2 + 1)
    return [c1, p1, p2, p2, p2]


def _lpips_package_dirs() -> List[str]:
    """the directories of an installed lpips package, found without importing it"""
    try:
        spec = importlib.util.find_spec("lpips")
    except (ImportError, ValueError):
        spec = None
    return list(spec.submodule_search_locations) if spec is not None and spec.submodule_search_locations else []


def lin_weight_candidates(net: str) -> List[str]:
    """where the linear heads are looked for: the installed lpips package's own file, then ``lpips-v0.1-<net>.pth`` in the hub
    checkpoint directories"""
    return ([os.path.join(d, "weights", "v0.1", f"{net}.pth") for d in _lpips_package_dirs()]
            + [os.path.join(d, f"lpips-v0.1-{net}.pth") for d in hub_checkpoint_dirs()])


class _LpipsHandle(L.Handle):
    """One ``mvd_lpips_t``; ``workspace(device, images, h, w)``."""

    def __init__(self):
        super().__init__("lpips")


def lpips_head(xs, ys, lin_w, relu_in=None, per_layer: bool = False, ws: Optional[torch.Tensor] = None, mean: bool = False):
    """``mvd_op_lpips_head``: xs[l], ys[l] (pairs, ..., C_l) channel-last maps, bf16 or fp32 (``relu_in[l]``: max(., 0) on an fp32 map
    on the way in), lin_w[l] (C_l,) fp32 >= 0 -> (per-pair distances (pairs,), per-layer terms (pairs, layers) or None, workspace).
    ``mean=True``: the first element is the mean over the pairs instead, a 0-d tensor (``mean_out`` alone: no per-pair output).
    One launch over all layers plus a one-workgroup finish."""
    n = len(xs)
    relu_in = list(relu_in) if relu_in is not None else [False] * n
    pairs = xs[0].shape[0]
    for a, b, w in zip(xs, ys, lin_w):
        assert a.is_cuda and a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == b.dtype, "lpips_head: contiguous CUDA maps of one shape"
        assert a.dtype in (torch.bfloat16, torch.float32) and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == a.shape[-1]
    pixels = (C.c_int * n)(*[a.numel() // (pairs * a.shape[-1]) for a in xs])
    chans = (C.c_int * n)(*[a.shape[-1] for a in xs])
    nbytes = L.check(L.lib().mvd_op_lpips_head_ws_bytes(n, pixels, pairs), "mvd_op_lpips_head_ws_bytes")
    if ws is None or ws.numel() < nbytes or ws.device != xs[0].device:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xs[0].device)
    out = torch.empty((() if mean else (pairs,)), device=xs[0].device, dtype=torch.float32)
    layers = torch.empty(pairs, n, device=xs[0].device, dtype=torch.float32) if per_layer else None
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    L.call("mvd_op_lpips_head", n, ptrs(xs), ptrs(ys), (C.c_int * n)(*[int(a.dtype == torch.bfloat16) for a in xs]),
           (C.c_int * n)(*[int(bool(r)) for r in relu_in]), pixels, chans, ptrs(lin_w), pairs,
           None if mean else C.c_void_p(out.data_ptr()), C.c_void_p(layers.data_ptr()) if per_layer else None,
           C.c_void_p(out.data_ptr()) if mean else None, C.c_void_p(ws.data_ptr()), ws.numel(), L.stream())
    return out, layers, ws


class LPIPS:
    """``lpips.LPIPS(net="alex" | "vgg")``: ``metric(x, y)`` -> (B, 1, 1, 1) fp32 on the device for image batches in [-1, 1]
    (``normalize=True``: in [0, 1]).  ``backbone``: the AlexNet / VGG-16 weights (state dict, ``.pth`` / ``.safetensors`` path, or
    ``None`` for torchvision's checkpoint in the local hub cache); ``model_path``: the linear heads (state dict, path, or ``None``
    for the lpips package's own file).  A full ``lpips.LPIPS(...).state_dict()`` serves as either, and then as both.
    ``max_pairs_per_pass`` is the pass size: larger batches run in several passes of that many pairs (and a shorter last one)
    within one call, whatever workspace earlier calls left behind, so the same inputs give the same bits on the same object."""

    def __init__(self, net: str = "alex", version: str = "0.1", spatial: bool = False, model_path=None, backbone=None, device="cuda",
                 max_pairs_per_pass: int = 8, **kw):
        who = "LPIPS"
        if net == "squeeze":
            raise L.MvdError(f"{who}: net='squeeze' is not built here (alex and vgg are)")
        if net not in ("alex", "vgg"):
            raise L.MvdError(f"{who}: net={net!r}: 'alex' or 'vgg'")
        if str(version) != "0.1":
            raise L.MvdError(f"{who}: version={version!r}: only the v0.1 heads and scaling layer exist here")
        if spatial:
            raise L.MvdError(f"{who}: spatial=True (a distance map per pixel) is not built here")
        for k, v in kw.items():
            if k not in _LPIPS_DEFAULTS:
                raise L.MvdError(f"{who}: unknown argument {k!r}")
            if bool(v) != _LPIPS_DEFAULTS[k] and k in ("lpips", "pnet_rand", "pnet_tune", "pretrained"):
                raise L.MvdError(f"{who}: {k}={v!r}: only the pretrained, linearly calibrated metric exists here ({k}={_LPIPS_DEFAULTS[k]})")
        if int(max_pairs_per_pass) < 1:
            raise L.MvdError(f"{who}: max_pairs_per_pass={max_pairs_per_pass!r} must be at least 1")
        self.net, self.device, self.max_pairs_per_pass = net, device, int(max_pairs_per_pass)
        self.chns = list(TAP_CHANNELS[net])
        both = None      # a full lpips state dict given as one argument serves the other too
        for given in (backbone, model_path):
            if given is not None and hasattr(given, "keys") and any(k.startswith("net.slice") for k in given.keys()) \
                    and any(k.startswith("lin") for k in given.keys()):
                both = given
        bb = resolve_state_dict(backbone if backbone is not None else both, [os.path.join(d, _BACKBONE_FILE[net]) for d in hub_checkpoint_dirs()],
                                who, f"{net} backbone ({_BACKBONE_FILE[net]})")
        lin = resolve_state_dict(model_path if model_path is not None else both, lin_weight_candidates(net), who, f"linear-head ({net}.pth)")
        convs = ALEX_CONVS if net == "alex" else VGG16_CONVS
        self.backbone = normalize_backbone_keys(bb, convs, "AlexNet" if net == "alex" else "VGG-16")
        self.lins = normalize_lpips_lin_keys(lin, self.chns)
        self._handle: Optional[_LpipsHandle] = None
        self._packed: Dict[str, torch.Tensor] = {}
        self._dev = None
        self._vgg: Optional[VGG16FeaturesHIP] = None
        self._head_ws: Optional[torch.Tensor] = None
        if net == "vgg":
            self._vgg = VGG16FeaturesHIP()
            self._vgg.load_state_dict(self.backbone)

    def to(self, device):
        self.device = device
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def _sync(self, dev: torch.device):
        if self._dev == dev:
            return
        if self.net == "alex":
            if self._handle is None:
                self._handle = _LpipsHandle()
            self._packed = pack_alex(self.backbone, self.lins, dev)
            self._handle.set_weights(self._packed)
        else:
            self._packed = {k: v.to(device=dev, dtype=torch.float32).contiguous() for k, v in self.lins.items()}
        self._dev = dev

    def _images(self, t, normalize: bool) -> torch.Tensor:
        who = f"LPIPS({self.net})"
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
            raise L.MvdError(f"{who}: images must be a (B, 3, H, W) tensor, got {tuple(getattr(t, 'shape', ()))}")
        lo = MIN_SIZE[self.net]
        if t.shape[2] < lo or t.shape[3] < lo:
            raise L.MvdError(f"{who}: images of {t.shape[2]} x {t.shape[3]} are smaller than the tower's pools need ({lo} x {lo})")
        if not t.is_cuda:
            raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): got a tensor on {t.device}; there is no CPU fallback")
        t = t.detach().to(torch.float32)
        return (2 * t - 1).contiguous() if normalize else t.contiguous()

    def features(self, images: torch.Tensor) -> List[torch.Tensor]:
        """the five post-ReLU taps of ``images`` (B, 3, H, W) in [-1, 1] as NCHW views: bf16, except the fifth of ``net="vgg"``
        (fp32, the ReLU applied here)"""
        x = self._images(images, False)
        self._sync(x.device)
        b, _, h, w = x.shape
        if self.net == "vgg":
            feat, taps = self._vgg(x, taps=True)
            return [taps[n] for n in TAP_NAMES] + [feat.clamp_min(0.0)]
        self._handle.workspace(x.device, b, h, w)
        taps = [torch.empty(b, th, tw, c, device=x.device, dtype=torch.bfloat16) for (th, tw), c in zip(alex_tap_sizes(h, w), self.chns)]
        L.call("mvd_lpips_features", self._handle.h, C.c_void_p(x.data_ptr()), b, h, w, (C.c_void_p * 5)(*[t.data_ptr() for t in taps]), L.stream())
        return [t.permute(0, 3, 1, 2) for t in taps]

    @torch.no_grad()
    def forward(self, in0, in1, retPerLayer: bool = False, normalize: bool = False):
        x, y = self._images(in0, normalize), self._images(in1, normalize)
        if x.shape != y.shape or x.device != y.device:
            raise L.MvdError(f"LPIPS: in0 {tuple(x.shape)} on {x.device} and in1 {tuple(y.shape)} on {y.device} must match")
        if x.device != torch.device(self.device):      # lpips follows its input's device
            self.to(x.device)
        self._sync(x.device)
        b, _, h, w = x.shape
        out = torch.empty(b, device=x.device, dtype=torch.float32)
        layers = torch.empty(b, 5, device=x.device, dtype=torch.float32) if retPerLayer else None
        if self.net == "alex":
            self._handle.workspace(x.device, 2 * min(b, self.max_pairs_per_pass), h, w)
            L.call("mvd_lpips_distance", self._handle.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), b, h, w, self.max_pairs_per_pass,
                   C.c_void_p(out.data_ptr()),
                   C.c_void_p(layers.data_ptr()) if retPerLayer else None, None, L.stream())
        else:
            pp = self.max_pairs_per_pass
            lin_w = [self._packed[f"lin{k}.weight"] for k in range(5)]
            for p0 in range(0, b, pp):
                n = min(pp, b - p0)
                feat, taps = self._vgg(torch.cat([x[p0:p0 + n], y[p0:p0 + n]]), taps=True)
                maps = [taps[name].permute(0, 2, 3, 1) for name in TAP_NAMES] + [feat.permute(0, 2, 3, 1)]      # the NHWC buffers themselves
                d, dl, self._head_ws = lpips_head([m[:n] for m in maps], [m[n:] for m in maps], lin_w, relu_in=[False] * 4 + [True],
                                                  per_layer=retPerLayer, ws=self._head_ws)
                out[p0:p0 + n] = d
                if retPerLayer:
                    layers[p0:p0 + n] = dl
        val = out.view(b, 1, 1, 1)
        return (val, [layers[:, k].reshape(b, 1, 1, 1) for k in range(5)]) if retPerLayer else val

    __call__ = forward

    @torch.no_grad()
    def mean_distance(self, in0, in1, normalize: bool = False) -> torch.Tensor:
        """the mean of ``metric(in0, in1)`` over the batch as a 0-d device tensor (what val.py:151 takes with ``.mean()``).  For
        ``net="alex"`` the finish kernel forms it in fp64 over all passes of the call; no per-pair values are written."""
        if self.net != "alex":
            return self.forward(in0, in1, normalize=normalize).double().mean().float()
        x, y = self._images(in0, normalize), self._images(in1, normalize)
        if x.shape != y.shape or x.device != y.device:
            raise L.MvdError(f"LPIPS: in0 {tuple(x.shape)} on {x.device} and in1 {tuple(y.shape)} on {y.device} must match")
        self._sync(x.device)
        b, _, h, w = x.shape
        mean = torch.empty((), device=x.device, dtype=torch.float32)
        self._handle.workspace(x.device, 2 * min(b, self.max_pairs_per_pass), h, w)
        L.call("mvd_lpips_distance", self._handle.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), b, h, w, self.max_pairs_per_pass,
               None, None, C.c_void_p(mean.data_ptr()), L.stream())
        return mean
