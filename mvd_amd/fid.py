"""FID on the MI355X: ``torchmetrics.image.fid.FrechetInceptionDistance(feature=2048)`` of the
reference's val.py without torchmetrics or torch-fidelity, on the HIP kernels of libmvd_hip.so (``mvd_fid_*``, csrc/fid.hip).

* ``InceptionV3FeaturesHIP`` -- the FID variant of Inception-v3 up to pool3 (torch-fidelity's ``FeatureExtractorInceptionV3``,
  pytorch-fid's ``pt_inception-2015-12-05``): uint8 (or fp32 in [0, 1]) images of any size -> (B, 2048) fp32.  The layer table
  is ``packing.INCEPTION_FID_LAYERS``; BatchNorm is folded on the host, the folded weights are stored in bf16.
* ``FrechetInceptionDistance`` -- torchmetrics' protocol (``.to``, ``update(imgs, real)``, ``compute()``, ``reset()``) and its
  six state tensors under its names.  ``update`` runs the tower and adds ``sum f`` and ``sum f f^T`` to the fp64 state on the GPU
  (``mvd_fid_update``); nothing synchronises until ``compute()``, which copies the state to the host and evaluates in fp64 there.
* ``fid_from_statistics(mu1, sigma1, mu2, sigma2)`` -- the Frechet distance of two Gaussians of any dimension.

The state tensors are plain sums, so a caller may all-reduce them across ranks before ``compute()``; that reduction is not
built here.  Nothing is ever fetched: the weights come from a state dict, a ``.pth`` / ``.safetensors`` path, or
``weights-inception-2015-12-05-6726825d.pth`` / ``pt_inception-2015-12-05-6726825d.pth`` in the local hub cache.  CPU tensors raise
``MvdError``: there is no fallback.  KID and the Inception score run on the same pool3 features: ``mvd_amd.kid`` (row N11); one
``InceptionV3FeaturesHIP`` can feed all three metrics (``inception=``, ``update_features``).  What is not here:
``feature=64 / 192 / 768``, a backward pass.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch

from . import _lib as L
from .packing import fid_program, inception_fc_weight, normalize_inception_fid_keys, pack_inception_fid
from .hub import hub_checkpoint_dirs, resolve_state_dict

INCEPTION_FID_FILES = ("weights-inception-2015-12-05-6726825d.pth", "pt_inception-2015-12-05-6726825d.pth")
FEATURE_DIM = 2048


def inception_weight_candidates():
    return [os.path.join(d, f) for d in hub_checkpoint_dirs() for f in INCEPTION_FID_FILES]


def load_inception_fid_weights(weights=None) -> Dict[str, torch.Tensor]:
    """A state dict from ``weights``: a dict as it is, a ``.pth`` / ``.safetensors`` path, or ``None`` = the first of
    ``INCEPTION_FID_FILES`` in the local hub cache.  Never downloads: a file that is not there raises ``MvdError``."""
    return resolve_state_dict(weights, inception_weight_candidates(), "InceptionV3FeaturesHIP", "Inception-v3 (FID) weight")


class _FidHandle(L.Handle):
    """One ``mvd_fid_t`` (the program of ``packing.fid_program``); ``workspace_bytes(images)``, ``workspace(device, images)``."""

    def __init__(self, max_images_per_pass: int):
        prog, bufs, names, final = fid_program()
        n_ops, n_bufs = len(prog) // 13, len(bufs) // 2
        super().__init__("fid", (C.c_int * len(prog))(*prog), n_ops, (C.c_int * len(bufs))(*bufs), n_bufs,
                         (C.c_char_p * len(names))(*[n.encode() for n in names]), len(names), final, int(max_images_per_pass))


class InceptionV3FeaturesHIP:
    """pool3 features of the FID Inception-v3: ``net(images)`` -> (B, 2048) fp32 on the device.  ``images``: (B, 3, H, W) uint8, or
    floating point in [0, 1] (quantised as torchmetrics' ``normalize=True`` does: ``x * 255`` in fp32, truncated; values outside
    [0, 1] are clamped).  ``max_images_per_pass`` is the pass size: larger batches run as several passes within one call; an
    image's features do not depend on the batch or the pass it is in.  ``fc_weight``: the classifier's (1008, 2048) fp32 weight when
    the state dict has one (``None`` otherwise); ``logits(pool3)`` applies it without the bias (``mvd_op_fc_logits``)."""

    def __init__(self, weights=None, max_images_per_pass: int = 8):
        if int(max_images_per_pass) < 1:
            raise L.MvdError(f"InceptionV3FeaturesHIP: max_images_per_pass={max_images_per_pass!r} must be at least 1")
        self.max_images_per_pass = int(max_images_per_pass)
        sd = load_inception_fid_weights(weights)
        self.state = normalize_inception_fid_keys(sd)
        self.fc_weight: Optional[torch.Tensor] = inception_fc_weight(sd, required=False)
        self._fc_dev: Optional[torch.Tensor] = None
        self._handle: Optional[_FidHandle] = None
        self._packed: Dict[str, torch.Tensor] = {}
        self._dev = None

    def to(self, *args, **kwargs):
        return self

    def eval(self):
        return self

    def _sync(self, dev: torch.device):
        if self._dev == dev:
            return
        if self._handle is None:
            self._handle = _FidHandle(self.max_images_per_pass)
        self._packed = pack_inception_fid(self.state, dev)
        self._handle.set_weights(self._packed)
        self._dev = dev

    def _images(self, t) -> torch.Tensor:
        who = "InceptionV3FeaturesHIP"
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1 or t.shape[2] < 1 or t.shape[3] < 1:
            raise L.MvdError(f"{who}: images must be a (B, 3, H, W) tensor, got {tuple(getattr(t, 'shape', ()))}")
        if not t.is_cuda:
            raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): got a tensor on {t.device}; there is no CPU fallback")
        if t.dtype != torch.uint8:
            if not t.is_floating_point():
                raise L.MvdError(f"{who}: images must be uint8 or floating point in [0, 1], got {t.dtype}")
            t = t.to(torch.float32)
        t = t.detach().contiguous()
        self._sync(t.device)
        return t

    @torch.no_grad()
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        x = self._images(images)
        b, _, h, w = x.shape
        self._handle.workspace(x.device, b)
        out = torch.empty(b, FEATURE_DIM, device=x.device, dtype=torch.float32)
        L.call("mvd_fid_features", self._handle.h, C.c_void_p(x.data_ptr()), int(x.dtype == torch.float32), b, h, w, C.c_void_p(out.data_ptr()), L.stream())
        return out

    __call__ = forward

    @torch.no_grad()
    def logits(self, pool3: torch.Tensor) -> torch.Tensor:
        """(b, 2048) fp32 pool3 features -> (b, 1008) fp32 ``logits_unbiased``: pool3 . fc.weight^T in fp32, no bias; a row's logits do
        not depend on the batch"""
        who = "InceptionV3FeaturesHIP.logits"
        if self.fc_weight is None:
            raise L.MvdError(f"{who}: the state dict has no 'fc.weight'")
        if not isinstance(pool3, torch.Tensor) or not pool3.is_cuda:
            raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): got a tensor on {getattr(pool3, 'device', None)}; there is no CPU fallback")
        if pool3.dim() != 2 or pool3.shape[1] != FEATURE_DIM or pool3.shape[0] < 1 or pool3.dtype != torch.float32:
            raise L.MvdError(f"{who}: features must be (b, {FEATURE_DIM}) fp32, got {tuple(pool3.shape)} {pool3.dtype}")
        f = pool3.detach().contiguous()
        if self._fc_dev is None or self._fc_dev.device != f.device:
            self._fc_dev = self.fc_weight.to(f.device)
        out = torch.empty(f.shape[0], self._fc_dev.shape[0], device=f.device, dtype=torch.float32)
        L.call("mvd_op_fc_logits", C.c_void_p(f.data_ptr()), f.shape[0], FEATURE_DIM, C.c_void_p(self._fc_dev.data_ptr()), self._fc_dev.shape[0],
               C.c_void_p(out.data_ptr()), L.stream())
        return out

    @torch.no_grad()
    def update_statistics(self, images: torch.Tensor, total: torch.Tensor, cov_sum: torch.Tensor) -> int:
        """features of ``images``, then in place ``total`` (2048,) += sum f and ``cov_sum`` (2048, 2048) += sum f f^T, both fp64 on the
        images' device (``mvd_fid_update``) -> the number of images"""
        x = self._images(images)
        for t, shape in ((total, (FEATURE_DIM,)), (cov_sum, (FEATURE_DIM, FEATURE_DIM))):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != x.device or not t.is_contiguous():
                raise L.MvdError(f"InceptionV3FeaturesHIP: the statistics must be contiguous fp64 tensors of {shape} on {x.device}")
        b, _, h, w = x.shape
        self._handle.workspace(x.device, b)
        L.call("mvd_fid_update", self._handle.h, C.c_void_p(x.data_ptr()), int(x.dtype == torch.float32), b, h, w, C.c_void_p(total.data_ptr()),
               C.c_void_p(cov_sum.data_ptr()), L.stream())
        return b


def fid_from_statistics(mu1, sigma1, mu2, sigma2) -> torch.Tensor:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2) in fp64 on the CPU, for any dimension -> a 0-d fp64 tensor.
    tr sqrt(S1 S2) = sum sqrt(max(lambda, 0)) over the eigenvalues of S1^(1/2) S2 S1^(1/2), with S1^(1/2) from ``eigh``: the matrix
    is real and symmetric and has the eigenvalues of S1 S2 (torchmetrics takes ``eigvals(S1 S2).sqrt().real.sum()``), and the form
    stays real for the rank-deficient covariances that few samples give.  Eigenvalues below d eps max(lambda) -- the rounding noise
    of a d x d symmetric eigenproblem, in S1 and in the product alike -- count as zero: the square root of such noise is 1e-8 of
    the scale, and d - rank of them would add up to 1e-5 of the result."""
    mu1, mu2 = (torch.as_tensor(m).detach().to("cpu", torch.float64).reshape(-1) for m in (mu1, mu2))
    s1, s2 = (torch.as_tensor(s).detach().to("cpu", torch.float64) for s in (sigma1, sigma2))
    d = mu1.numel()
    if mu2.numel() != d or tuple(s1.shape) != (d, d) or tuple(s2.shape) != (d, d):
        raise ValueError(f"fid_from_statistics: means of {mu1.numel()} and {mu2.numel()}, covariances {tuple(s1.shape)} and {tuple(s2.shape)}")
    noise = d * torch.finfo(torch.float64).eps

    def floor_noise(ev):
        return torch.where(ev > noise * ev.max().clamp_min(0.0), ev, torch.zeros_like(ev))

    s1, s2 = 0.5 * (s1 + s1.T), 0.5 * (s2 + s2.T)
    lam, vec = torch.linalg.eigh(s1)
    root = (vec * floor_noise(lam).sqrt()) @ vec.T
    m = root @ s2 @ root
    ev = torch.linalg.eigvalsh(0.5 * (m + m.T))
    tr_root = floor_noise(ev).sqrt().sum()
    diff = mu1 - mu2
    return diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2.0 * tr_root


def statistics_from_sums(total, cov_sum, n: int):
    """torchmetrics' compute(): mu = sum / n, Sigma = (cov_sum - n mu mu^T) / (n - 1), fp64 on the CPU"""
    total, cov_sum = total.detach().to("cpu", torch.float64), cov_sum.detach().to("cpu", torch.float64)
    mu = total / n
    return mu, (cov_sum - n * torch.outer(mu, mu)) / (n - 1)


class FrechetInceptionDistance:
    """``torchmetrics.image.fid.FrechetInceptionDistance(feature=2048)`` on this project's kernels.  ``update(imgs, real)``: uint8
    images, or (``normalize=True``) floating point in [0, 1]; ``compute()`` -> the FID as a 0-d fp64 device tensor -- the one place
    that synchronises: the six state tensors go to the host and the distance is evaluated in fp64 there (``fid_from_statistics``).
    ``reset()`` keeps the real statistics when ``reset_real_features=False``.  ``weights``: see ``load_inception_fid_weights``.
    ``inception``: an ``InceptionV3FeaturesHIP`` shared with other metrics (then ``weights`` and ``max_images_per_pass`` are not used);
    ``update_features(pool3, real)`` adds the statistics of features from a tower call made elsewhere."""

    STATE = ("real_features_sum", "real_features_cov_sum", "real_features_num_samples", "fake_features_sum", "fake_features_cov_sum",
             "fake_features_num_samples")

    def __init__(self, feature=2048, reset_real_features: bool = True, normalize: bool = False, weights=None, max_images_per_pass: int = 8,
                 device="cuda", inception=None):
        if isinstance(feature, bool) or not isinstance(feature, int) or feature != FEATURE_DIM:
            raise ValueError(f"FrechetInceptionDistance: feature={feature!r}: only the 2048 pool3 features are built here "
                             "(not 64 / 192 / 768, not a custom module)")
        if not isinstance(reset_real_features, bool) or not isinstance(normalize, bool):
            raise ValueError("FrechetInceptionDistance: reset_real_features and normalize must be bool")
        if inception is not None and not isinstance(inception, InceptionV3FeaturesHIP):
            raise ValueError(f"FrechetInceptionDistance: inception must be an InceptionV3FeaturesHIP, got {type(inception).__name__}")
        self.inception = inception if inception is not None else InceptionV3FeaturesHIP(weights, max_images_per_pass=max_images_per_pass)
        self.reset_real_features, self.normalize = reset_real_features, normalize
        self.device = torch.device(device)
        self._allocate(("real", "fake"))

    def _allocate(self, sides):
        dev = self.device if self.device.type == "cuda" and torch.cuda.is_available() else torch.device("cpu")
        for side in sides:
            setattr(self, f"{side}_features_sum", torch.zeros(FEATURE_DIM, dtype=torch.float64, device=dev))
            setattr(self, f"{side}_features_cov_sum", torch.zeros(FEATURE_DIM, FEATURE_DIM, dtype=torch.float64, device=dev))
            setattr(self, f"{side}_features_num_samples", torch.zeros((), dtype=torch.long, device=dev))

    def to(self, device=None, *args, **kwargs):
        if device is not None and not isinstance(device, torch.dtype):
            device = torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if device != self.real_features_sum.device:
                for name in self.STATE:
                    setattr(self, name, getattr(self, name).to(device))
            self.device = device
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool) -> None:
        who = "FrechetInceptionDistance.update"
        if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
            raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): pass CUDA tensors; there is no CPU fallback")
        if self.normalize:
            if not imgs.is_floating_point():
                raise L.MvdError(f"{who}: normalize=True takes floating-point images in [0, 1], got {imgs.dtype}")
        elif imgs.dtype != torch.uint8:
            raise L.MvdError(f"{who}: normalize=False takes uint8 images, got {imgs.dtype}")
        if self.real_features_sum.device != imgs.device:
            self.to(imgs.device)
        side = "real" if real else "fake"
        n = self.inception.update_statistics(imgs, getattr(self, f"{side}_features_sum"), getattr(self, f"{side}_features_cov_sum"))
        getattr(self, f"{side}_features_num_samples").add_(n)

    @torch.no_grad()
    def update_features(self, pool3: torch.Tensor, real: bool) -> None:
        """the statistics of given (b, 2048) fp32 pool3 features (``mvd_op_feature_stats``): what ``update`` adds behind the tower"""
        who = "FrechetInceptionDistance.update_features"
        if not isinstance(pool3, torch.Tensor) or not pool3.is_cuda:
            raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): pass CUDA tensors; there is no CPU fallback")
        if pool3.dim() != 2 or pool3.shape[1] != FEATURE_DIM or pool3.shape[0] < 1 or pool3.dtype != torch.float32:
            raise L.MvdError(f"{who}: features must be (b, {FEATURE_DIM}) fp32, got {tuple(pool3.shape)} {pool3.dtype}")
        if self.real_features_sum.device != pool3.device:
            self.to(pool3.device)
        f = pool3.detach().contiguous()
        side = "real" if real else "fake"
        L.call("mvd_op_feature_stats", C.c_void_p(f.data_ptr()), f.shape[0], FEATURE_DIM, C.c_void_p(getattr(self, f"{side}_features_sum").data_ptr()),
               C.c_void_p(getattr(self, f"{side}_features_cov_sum").data_ptr()), L.stream())
        getattr(self, f"{side}_features_num_samples").add_(f.shape[0])

    def compute(self) -> torch.Tensor:
        host = {name: getattr(self, name).detach().cpu() for name in self.STATE}      # the synchronisation of this protocol
        n_real, n_fake = int(host["real_features_num_samples"]), int(host["fake_features_num_samples"])
        if n_real < 2 or n_fake < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        mu_r, sig_r = statistics_from_sums(host["real_features_sum"], host["real_features_cov_sum"], n_real)
        mu_f, sig_f = statistics_from_sums(host["fake_features_sum"], host["fake_features_cov_sum"], n_fake)
        return fid_from_statistics(mu_r, sig_r, mu_f, sig_f).to(self.real_features_sum.device)

    def reset(self) -> None:
        for side in ("real", "fake") if self.reset_real_features else ("fake",):
            for leaf in ("sum", "cov_sum", "num_samples"):
                getattr(self, f"{side}_features_{leaf}").zero_()

    def __call__(self, imgs: torch.Tensor, real: bool) -> None:
        self.update(imgs, real)
