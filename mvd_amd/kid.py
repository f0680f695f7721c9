"""KID and the Inception score on the MI355X: ``torchmetrics.image.kid.KernelInceptionDistance`` and
``torchmetrics.image.inception.InceptionScore(feature="logits_unbiased")`` without torchmetrics or torch-fidelity, on the pool3
features of ``mvd_amd.fid.InceptionV3FeaturesHIP`` and the kernels of csrc/kid.hip.

* ``KernelInceptionDistance`` -- torchmetrics' protocol and state (``real_features`` / ``fake_features``: lists of (b, 2048) fp32
  device tensors).  ``compute()`` draws the subsets on the host exactly as torchmetrics does (``kid_subsets``), uploads ONE int32
  tensor and launches ``mvd_op_kid_mmd`` once: the polynomial-kernel MMD of every subset in fp64 on the f64 MFMA, no m x m
  matrix, a fixed summation order -> ``(mean, std)`` as 0-d fp64 device tensors.
* ``InceptionScore`` -- the state is ``features``, a list of (b, 1008) fp32 logits = pool3 . ``fc.weight``^T without the bias
  (``mvd_op_fc_logits``); ``compute()`` shuffles with ``torch.randperm`` and runs the head in fp64 (``mvd_op_inception_score``).
* One tower can feed FID, KID and the Inception score: build ``InceptionV3FeaturesHIP`` once, pass it as ``inception=`` and call
  ``update_features(pool3, ...)`` on each metric.

CPU tensors raise ``MvdError``, nothing is ever fetched, and ``compute()`` is the only call that synchronises.  What is not
here: ``feature=64 / 192 / 768``, the ``logits`` (biased) and ``2048`` variants of the Inception score, gathering the feature
lists across ranks, a backward pass.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from . import _lib as L
from .fid import FEATURE_DIM, InceptionV3FeaturesHIP

NUM_CLASSES = 1008


def _is_pos_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and v > 0


def kid_subsets(n_real: int, n_fake: int, subsets: int, m: int) -> torch.Tensor:
    """(subsets, 2, m) int32 on the CPU: per subset ``torch.randperm(n_real)[:m]`` then ``torch.randperm(n_fake)[:m]`` from the global
    CPU generator -- the draws of torchmetrics' ``compute()`` in its order, so a seeded run picks the same subsets"""
    if m < 2:
        raise ValueError(f"Argument `subset_size` should be at least 2 for the unbiased estimate, got {m}")
    if m > n_real or m > n_fake:
        raise ValueError("Argument `subset_size` should be smaller than the number of samples")
    out = torch.empty(subsets, 2, m, dtype=torch.int32)
    for s in range(subsets):
        out[s, 0] = torch.randperm(n_real)[:m]
        out[s, 1] = torch.randperm(n_fake)[:m]
    return out


def chunk_bounds(n: int, splits: int) -> List[Tuple[int, int]]:
    """the [start, end) row ranges of ``torch.chunk(splits)`` over n rows: ceil(n / splits) rows each, the last one shorter,
    possibly fewer than ``splits`` of them"""
    size = -(-n // splits)
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _features(t, width, who) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): pass CUDA tensors; there is no CPU fallback")
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1 or t.dtype != torch.float32:
        raise L.MvdError(f"{who}: features must be (b, {width}) fp32, got {tuple(t.shape)} {t.dtype}")
    return t.detach().contiguous()


def _check_images(imgs, normalize, who):
    if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): pass CUDA tensors; there is no CPU fallback")
    if normalize:
        if not imgs.is_floating_point():
            raise L.MvdError(f"{who}: normalize=True takes floating-point images in [0, 1], got {imgs.dtype}")
    elif imgs.dtype != torch.uint8:
        raise L.MvdError(f"{who}: normalize=False takes uint8 images, got {imgs.dtype}")


def _tower(inception, weights, max_images_per_pass, who):
    if inception is None:
        return InceptionV3FeaturesHIP(weights, max_images_per_pass=max_images_per_pass)
    if not isinstance(inception, InceptionV3FeaturesHIP):
        raise ValueError(f"{who}: inception must be an InceptionV3FeaturesHIP, got {type(inception).__name__}")
    return inception


class KernelInceptionDistance:
    """``torchmetrics.image.kid.KernelInceptionDistance(feature=2048)`` on this project's kernels.  ``update(imgs, real)``: uint8
    images, or (``normalize=True``) floating point in [0, 1]; ``update_features(pool3, real)``: features of a tower call made
    elsewhere; ``compute()`` -> ``(mean, std)`` of the subsets' MMD, 0-d fp64 device tensors.  ``gamma=None`` is 1 / 2048.
    ``inception``: a shared ``InceptionV3FeaturesHIP`` (then ``weights`` and ``max_images_per_pass`` are not used)."""

    def __init__(self, feature=2048, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma=None, coef: float = 1.0,
                 reset_real_features: bool = True, normalize: bool = False, weights=None, inception=None, max_images_per_pass: int = 8, device="cuda"):
        if isinstance(feature, bool) or not isinstance(feature, int) or feature != FEATURE_DIM:
            raise ValueError(f"KernelInceptionDistance: feature={feature!r}: only the 2048 pool3 features are built here "
                             "(not 64 / 192 / 768, not a custom module)")
        if not _is_pos_int(subsets):
            raise ValueError("Argument `subsets` expected to be integer larger than 0")
        if not _is_pos_int(subset_size):
            raise ValueError("Argument `subset_size` expected to be integer larger than 0")
        if not _is_pos_int(degree):
            raise ValueError("Argument `degree` expected to be integer larger than 0")
        if gamma is not None and not (isinstance(gamma, float) and gamma > 0):
            raise ValueError("Argument `gamma` expected to be `None` or float larger than 0")
        if not (isinstance(coef, float) and coef > 0):
            raise ValueError("Argument `coef` expected to be float larger than 0")
        if not isinstance(reset_real_features, bool):
            raise ValueError("Argument `reset_real_features` expected to be a bool")
        if not isinstance(normalize, bool):
            raise ValueError("Argument `normalize` expected to be a bool")
        self.inception = _tower(inception, weights, max_images_per_pass, "KernelInceptionDistance")
        self.subsets, self.subset_size, self.degree, self.gamma, self.coef = subsets, subset_size, degree, gamma, coef
        self.reset_real_features, self.normalize = reset_real_features, normalize
        self.device = torch.device(device)
        self.real_features: List[torch.Tensor] = []
        self.fake_features: List[torch.Tensor] = []

    def to(self, device=None, *args, **kwargs):
        if device is not None and not isinstance(device, torch.dtype):
            self.device = torch.device(device)
            self.real_features = [t.to(self.device) for t in self.real_features]
            self.fake_features = [t.to(self.device) for t in self.fake_features]
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    @torch.no_grad()
    def update_features(self, pool3: torch.Tensor, real: bool) -> None:
        (self.real_features if real else self.fake_features).append(_features(pool3, FEATURE_DIM, "KernelInceptionDistance.update_features"))

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool) -> None:
        _check_images(imgs, self.normalize, "KernelInceptionDistance.update")
        self.update_features(self.inception(imgs), real)

    def compute(self):
        if not self.real_features or not self.fake_features:
            raise ValueError("Argument `subset_size` should be smaller than the number of samples")
        f_real, f_fake = torch.cat(self.real_features), torch.cat(self.fake_features)
        idx = kid_subsets(f_real.shape[0], f_fake.shape[0], self.subsets, self.subset_size)      # raises before any launch
        from . import ops
        scores = ops.kid_mmd(f_real, f_fake.to(f_real.device), idx.to(f_real.device), self.degree, self.gamma, self.coef)
        return scores.mean(), scores.std(unbiased=False)

    def reset(self) -> None:
        if self.reset_real_features:
            self.real_features = []
        self.fake_features = []

    def __call__(self, imgs: torch.Tensor, real: bool) -> None:
        self.update(imgs, real)


class InceptionScore:
    """``torchmetrics.image.inception.InceptionScore(feature="logits_unbiased")`` on this project's kernels.  ``update(imgs)``:
    uint8 images, or (``normalize=True``) floating point in [0, 1]; ``update_features(pool3)``: pool3 features of a tower call made
    elsewhere, turned into the 1008 logits here; ``compute()`` -> ``(mean, std)`` over the chunks' scores, 0-d fp64 device tensors
    (``std`` is ``torch.std``'s unbiased default: NaN for one chunk, as in torch).  The state dict must hold ``fc.weight``."""

    def __init__(self, feature="logits_unbiased", splits: int = 10, normalize: bool = False, weights=None, inception=None,
                 max_images_per_pass: int = 8, device="cuda"):
        if feature != "logits_unbiased":
            raise ValueError(f"InceptionScore: feature={feature!r}: only 'logits_unbiased' is built here (not 'logits', not a pool tap, "
                             "not a custom module)")
        if not _is_pos_int(splits):
            raise ValueError("Argument `splits` expected to be integer larger than 0")
        if not isinstance(normalize, bool):
            raise ValueError("Argument `normalize` expected to be a bool")
        self.inception = _tower(inception, weights, max_images_per_pass, "InceptionScore")
        if self.inception.fc_weight is None:
            raise L.MvdError("InceptionScore: the Inception-v3 state dict has no 'fc.weight': the Inception score needs the classifier "
                             "(FID and KID do not)")
        self.splits, self.normalize = splits, normalize
        self.device = torch.device(device)
        self.features: List[torch.Tensor] = []

    def to(self, device=None, *args, **kwargs):
        if device is not None and not isinstance(device, torch.dtype):
            self.device = torch.device(device)
            self.features = [t.to(self.device) for t in self.features]
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    @torch.no_grad()
    def update_features(self, pool3: torch.Tensor) -> None:
        f = _features(pool3, FEATURE_DIM, "InceptionScore.update_features")
        self.features.append(self.inception.logits(f))

    @torch.no_grad()
    def update(self, imgs: torch.Tensor) -> None:
        _check_images(imgs, self.normalize, "InceptionScore.update")
        self.update_features(self.inception(imgs))

    def compute(self):
        if not self.features:
            raise ValueError("InceptionScore.compute: no samples (call update first)")
        logits = torch.cat(self.features)
        perm = torch.randperm(logits.shape[0]).to(torch.int32)
        from . import ops
        kl = ops.inception_score_chunks(logits, perm.to(logits.device), self.splits)
        return kl.mean(), kl.std()

    def reset(self) -> None:
        self.features = []

    def __call__(self, imgs: torch.Tensor) -> None:
        self.update(imgs)
