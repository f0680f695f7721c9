"""Precision / recall and density / coverage on the MI355X: torch-fidelity's ``prc`` metric (improved
precision and recall, Kynkaanniemi et al. 2019) and the ``prdc`` package's density and coverage (Naeem et al. 2020) without either
package, on the pool3 features of ``mvd_amd.fid.InceptionV3FeaturesHIP`` and the kernels of csrc/prdc.hip.  FID and KID give
one number; these split it into fidelity (do the renders look like real views?) and diversity (do they cover the real views?).

All comparisons are on squared distances ``D2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b)`` in fp64 from the fp32 features;
``radii_k(F)[i]`` is the (k + 1)-th smallest value of row i of ``D2(F, F)``, the row itself included (``kthvalue(k + 1)``).

* ``PrecisionRecall`` (k = ``neighborhood`` = 3, closed comparison ``<=``; ``strict=True``: ``<``)::

      precision = #{j : exists i, D2(fake_j, real_i) <= radii_k(real)[i]} / n_fake
      recall    = #{i : exists j, D2(real_i, fake_j) <= radii_k(fake)[j]} / n_real
      f_score   = 2 p r / max(p + r, 1e-5)

* ``DensityCoverage`` (k = ``nearest_k`` = 5, strict comparison ``<``, radii of the real set only)::

      density  = sum_j #{i : D2(fake_j, real_i) < radii_k(real)[i]} / (k n_fake)
      coverage = #{i : exists j, D2(fake_j, real_i) < radii_k(real)[i]} / n_real

* ``knn_radii(features, k)`` and ``manifold_counts(query, ref, radii_sq, closed)`` expose the two operators: everything above is a
  row or column sum of one predicate matrix ``P[j][i] = D2(query_j, ref_i) (<= or <) radii(ref)[i]``, which is never stored.

Protocol, state names and tower sharing are ``KernelInceptionDistance``'s: ``real_features`` / ``fake_features`` are lists of
(b, 2048) fp32 device tensors; one ``InceptionV3FeaturesHIP`` passed as ``inception=`` and ``update_features(pool3, real)`` feed
FID, KID and these two from one tower call.  ``compute()`` returns 0-d fp64 device tensors formed with torch ops on the kernels'
int32 counts and synchronises nothing.  CPU tensors raise ``MvdError``; nothing is ever fetched.  What is not here: ``feature``
other than 2048, gathering the feature lists across ranks, perceptual path length and the realism score, a backward pass.
"""
from __future__ import annotations

from typing import List

import torch

from . import _lib as L
from .fid import FEATURE_DIM
from .kid import _check_images, _features, _tower

K_MAX = 15


def _is_k(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= K_MAX


def knn_radii(features: torch.Tensor, k: int) -> torch.Tensor:
    """(n, d) fp32 device features -> (n,) fp64 ``radii_k(features)``: squared distance to the k-th nearest OTHER row"""
    f = _features_any(features, "knn_radii")
    if not _is_k(k):
        raise ValueError(f"knn_radii: k must be an integer in [1, {K_MAX}], got {k!r}")
    if f.shape[0] < k + 1:
        raise ValueError(f"knn_radii: k = {k} needs at least {k + 1} samples, got {f.shape[0]}")
    from . import ops
    return ops.knn_radii(f, k)


def manifold_counts(query: torch.Tensor, ref: torch.Tensor, radii_sq: torch.Tensor, closed: bool):
    """-> (hits_per_query (nq,), hits_per_ref (nr,)) int32: the row and column sums of ``D2(query_j, ref_i) <= radii_sq[i]``
    (``closed``) or ``<`` (not ``closed``)"""
    q, r = _features_any(query, "manifold_counts"), _features_any(ref, "manifold_counts")
    if q.shape[1] != r.shape[1]:
        raise L.MvdError(f"manifold_counts: query and ref differ in width ({q.shape[1]}, {r.shape[1]})")
    if not isinstance(radii_sq, torch.Tensor) or not radii_sq.is_cuda or radii_sq.dtype != torch.float64 or radii_sq.shape != (r.shape[0],):
        raise L.MvdError(f"manifold_counts: radii_sq must be ({r.shape[0]},) fp64 on the GPU")
    from . import ops
    return ops.manifold_counts(q, r, radii_sq.contiguous(), bool(closed))


def _features_any(t, who) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.MvdError(f"{who} runs on the GPU only (libmvd_hip.so): pass CUDA tensors; there is no CPU fallback")
    if t.dim() != 2 or t.shape[0] < 1 or t.dtype != torch.float32:
        raise L.MvdError(f"{who}: features must be (n, d) fp32, got {tuple(t.shape)} {t.dtype}")
    return t.detach().contiguous()


def _ratio(count: torch.Tensor, denom: int) -> torch.Tensor:
    """count / denom as ONE IEEE fp64 division on the device (a tensor divided by a Python scalar is multiplied by the scalar's
    rounded reciprocal instead, which is off by an ulp for ratios such as 119 / 130)"""
    c = count.to(torch.float64)
    return c / torch.full_like(c, float(denom))


class _ManifoldMetric:
    """state and protocol shared by the two metrics (``KernelInceptionDistance``'s)"""

    def __init__(self, who, feature, reset_real_features, normalize, weights, inception, max_images_per_pass, device):
        if isinstance(feature, bool) or not isinstance(feature, int) or feature != FEATURE_DIM:
            raise ValueError(f"{who}: feature={feature!r}: only the 2048 pool3 features are built here (not 64 / 192 / 768, not a custom module)")
        if not isinstance(reset_real_features, bool):
            raise ValueError("Argument `reset_real_features` expected to be a bool")
        if not isinstance(normalize, bool):
            raise ValueError("Argument `normalize` expected to be a bool")
        self._who = who
        self.inception = _tower(inception, weights, max_images_per_pass, who)
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
        (self.real_features if real else self.fake_features).append(_features(pool3, FEATURE_DIM, f"{self._who}.update_features"))

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool) -> None:
        _check_images(imgs, self.normalize, f"{self._who}.update")
        self.update_features(self.inception(imgs), real)

    def reset(self) -> None:
        if self.reset_real_features:
            self.real_features = []
        self.fake_features = []

    def __call__(self, imgs: torch.Tensor, real: bool) -> None:
        self.update(imgs, real)

    def _sides(self, k, need_fake_radii):
        """the two feature matrices, after every check that can fail: nothing has been launched when this raises"""
        n_real, n_fake = (sum(t.shape[0] for t in side) for side in (self.real_features, self.fake_features))
        if n_real < k + 1:
            raise ValueError(f"{self._who}.compute: k = {k} needs at least {k + 1} real samples, got {n_real}")
        if n_fake < (k + 1 if need_fake_radii else 1):
            raise ValueError(f"{self._who}.compute: " + (f"k = {k} needs at least {k + 1} fake samples" if need_fake_radii else "no fake samples")
                             + f", got {n_fake}")
        real = torch.cat(self.real_features)
        return real, torch.cat(self.fake_features).to(real.device)


class PrecisionRecall(_ManifoldMetric):
    """torch-fidelity's ``prc`` metric (improved precision / recall) on this project's kernels.  ``update(imgs, real)``: uint8
    images, or (``normalize=True``) floating point in [0, 1]; ``update_features(pool3, real)``: features of a tower call made
    elsewhere; ``compute()`` -> ``(precision, recall, f_score)``, 0-d fp64 device tensors.  ``neighborhood``: torch-fidelity's
    ``prc_neighborhood``; ``strict=True``: the ``prdc`` package's ``<`` in place of ``<=``.  ``inception``: a shared
    ``InceptionV3FeaturesHIP`` (then ``weights`` and ``max_images_per_pass`` are not used)."""

    def __init__(self, feature=2048, neighborhood: int = 3, strict: bool = False, reset_real_features: bool = True, normalize: bool = False,
                 weights=None, inception=None, max_images_per_pass: int = 8, device="cuda"):
        if not _is_k(neighborhood):
            raise ValueError(f"Argument `neighborhood` expected to be an integer in [1, {K_MAX}]")
        if not isinstance(strict, bool):
            raise ValueError("Argument `strict` expected to be a bool")
        super().__init__("PrecisionRecall", feature, reset_real_features, normalize, weights, inception, max_images_per_pass, device)
        self.neighborhood, self.strict = neighborhood, strict

    def compute(self):
        real, fake = self._sides(self.neighborhood, need_fake_radii=True)
        from . import ops
        closed = not self.strict
        hits_fake, _ = ops.manifold_counts(fake, real, ops.knn_radii(real, self.neighborhood), closed, want_ref=False)
        hits_real, _ = ops.manifold_counts(real, fake, ops.knn_radii(fake, self.neighborhood), closed, want_ref=False)
        precision = _ratio((hits_fake > 0).sum(), fake.shape[0])
        recall = _ratio((hits_real > 0).sum(), real.shape[0])
        f_score = 2.0 * precision * recall / torch.clamp(precision + recall, min=1e-5)
        return precision, recall, f_score


class DensityCoverage(_ManifoldMetric):
    """the ``prdc`` package's density and coverage on this project's kernels; the protocol is ``PrecisionRecall``'s.
    ``compute()`` -> ``(density, coverage)``, 0-d fp64 device tensors (density may exceed 1).  ``nearest_k``: ``prdc``'s."""

    def __init__(self, feature=2048, nearest_k: int = 5, reset_real_features: bool = True, normalize: bool = False, weights=None, inception=None,
                 max_images_per_pass: int = 8, device="cuda"):
        if not _is_k(nearest_k):
            raise ValueError(f"Argument `nearest_k` expected to be an integer in [1, {K_MAX}]")
        super().__init__("DensityCoverage", feature, reset_real_features, normalize, weights, inception, max_images_per_pass, device)
        self.nearest_k = nearest_k

    def compute(self):
        real, fake = self._sides(self.nearest_k, need_fake_radii=False)
        from . import ops
        hits_fake, hits_real = ops.manifold_counts(fake, real, ops.knn_radii(real, self.nearest_k), False)
        density = _ratio(hits_fake.sum(), self.nearest_k * fake.shape[0])
        coverage = _ratio((hits_real > 0).sum(), real.shape[0])
        return density, coverage
