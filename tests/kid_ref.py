"""torchmetrics' ``KernelInceptionDistance`` and ``InceptionScore`` arithmetic restated in fp64 torch -- neither torchmetrics nor
torch-fidelity is installed where this project runs, so this file is what the kernels of csrc/kid.hip are compared with;
tests/test_kid_cpu.py checks it against the package where it imports.

* ``poly_kernel`` / ``maximum_mean_discrepancy`` / ``poly_mmd``: torchmetrics/image/kid.py, on fp64 copies of the features;
  ``mmd_terms`` gives the three sums and the term scale T = (|S_xx| + |S_yy|) / (m (m - 1)) + 2 |S_xy| / m^2 that every bound here
  is relative to (KID itself may be near zero); ``kid_scores`` draws the subsets as ``compute()`` does.
* ``inception_score_chunks``: ``InceptionScore.compute`` behind the shuffle, one score per chunk.
* ``integer_features``: rows over {-1, 0, 1}: with gamma = 1 / d a power of two every kernel value and every sum of them is
  exact in fp64 in ANY order (tests/test_kid_cpu.py::test_integer_inputs_are_exact), so the GPU comparison is ``torch.equal``.
* ``synthetic_inception_state_dict``: fid_ref's seeded state dict with a seeded ``fc.weight`` (fid_ref's is zero).

Plain helper module (like fid_ref.py), no fixtures."""
import functools
import math

import torch

import fid_ref as R

CLASSES = 1008
# maximum over seeds 0-2 of tests/test_kid_cpu.py::test_emulation_error_constant: |KID_emu - KID_fp32| / T for the bf16 emulation of
# the tower against the fp32 tower (four real + four fake 64 x 64 images, subset_size 3, 4 subsets, the default kernel)
KID_EMU_REL = 2.0e-6       # measured maximum 1.37e-6 (seed 0; per subset, T = 4.3 - 4.8, KID 4e-4 - 4e-3)
MEASURE = dict(subset_size=3, subsets=4)


# ------------------------------------------------------------------------------------------------ KID
def poly_kernel(f1, f2, degree=3, gamma=None, coef=1.0):
    if gamma is None:
        gamma = 1.0 / f1.shape[1]
    return (f1 @ f2.T * gamma + coef) ** degree


def maximum_mean_discrepancy(k_xx, k_xy, k_yy):
    m = k_xx.shape[0]
    kt_xx_sum = (k_xx.sum(dim=-1) - torch.diag(k_xx)).sum()
    kt_yy_sum = (k_yy.sum(dim=-1) - torch.diag(k_yy)).sum()
    k_xy_sum = k_xy.sum(dim=0).sum()
    value = (kt_xx_sum + kt_yy_sum) / (m * (m - 1))
    value -= 2 * k_xy_sum / (m ** 2)
    return value


def poly_mmd(f_real, f_fake, degree=3, gamma=None, coef=1.0):
    f_real, f_fake = f_real.detach().cpu().double(), f_fake.detach().cpu().double()
    return maximum_mean_discrepancy(poly_kernel(f_real, f_real, degree, gamma, coef), poly_kernel(f_real, f_fake, degree, gamma, coef),
                                    poly_kernel(f_fake, f_fake, degree, gamma, coef))


def mmd_terms(f_real, f_fake, degree=3, gamma=None, coef=1.0):
    """(S_xx, S_yy, S_xy, T) as Python floats: the off-diagonal sums of k_xx and k_yy, the full sum of k_xy, and the term scale"""
    x, y = f_real.detach().cpu().double(), f_fake.detach().cpu().double()
    m = x.shape[0]
    k_xx, k_yy, k_xy = poly_kernel(x, x, degree, gamma, coef), poly_kernel(y, y, degree, gamma, coef), poly_kernel(x, y, degree, gamma, coef)
    sxx, syy, sxy = float(k_xx.sum() - k_xx.diag().sum()), float(k_yy.sum() - k_yy.diag().sum()), float(k_xy.sum())
    absx = float(k_xx.abs().sum() - k_xx.diag().abs().sum())
    absy = float(k_yy.abs().sum() - k_yy.diag().abs().sum())
    scale = (absx + absy) / (m * (m - 1)) + 2 * float(k_xy.abs().sum()) / m ** 2
    return sxx, syy, sxy, scale


def mmd_bound(m, d, scale):
    """4 (m^2 + d) 2^-53 T: the worst-case fp64 summation error of both sides -- each side adds at most m^2 kernel values whose
    d-term dot products carry d roundings, 2^-53 relative each, against the sum of the absolute terms"""
    return 4.0 * (m * m + d) * 2.0 ** -53 * scale


def draw_subsets(n_real, n_fake, subsets, m):
    """the ``randperm`` sequence of torchmetrics' ``compute()``, written out: real then fake, per subset"""
    out = []
    for _ in range(subsets):
        a = torch.randperm(n_real)[:m]
        b = torch.randperm(n_fake)[:m]
        out.append((a, b))
    return out


def kid_scores(f_real, f_fake, subsets, m, degree=3, gamma=None, coef=1.0, draws=None):
    """per-subset MMD (fp64 tensor) and per-subset term scale T, over ``draws`` or fresh draws from the global generator"""
    draws = draw_subsets(f_real.shape[0], f_fake.shape[0], subsets, m) if draws is None else draws
    f_real, f_fake = f_real.detach().cpu(), f_fake.detach().cpu()
    vals = torch.stack([poly_mmd(f_real[a], f_fake[b], degree, gamma, coef) for a, b in draws])
    scales = [mmd_terms(f_real[a], f_fake[b], degree, gamma, coef)[3] for a, b in draws]
    return vals, scales


# ------------------------------------------------------------------------------------------------ the Inception score
def inception_score_chunks(logits, idx, splits):
    """``InceptionScore.compute`` behind ``idx = torch.randperm(n)``, in fp64 -> the stacked per-chunk scores (before mean / std)"""
    features = logits.detach().cpu().double()[idx]
    prob = features.softmax(dim=1)
    log_prob = features.log_softmax(dim=1)
    prob = prob.chunk(splits, dim=0)
    log_prob = log_prob.chunk(splits, dim=0)
    mean_prob = [p.mean(dim=0, keepdim=True) for p in prob]
    kl_ = [p * (log_p - m_p.log()) for p, log_p, m_p in zip(prob, log_prob, mean_prob)]
    kl_ = [k.sum(dim=1).mean().exp() for k in kl_]
    return torch.stack(kl_)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=8)
def integer_features(n, d, seed, max_nonzero=255):
    """(n, d) fp32 over {-1, 0, 1}, at most ``max_nonzero`` non-zeros a row -- computed once per process and shared; do not modify"""
    g = torch.Generator().manual_seed(4000 + seed)
    f = torch.zeros(n, d)
    for i in range(n):
        k = int(torch.randint(1, min(max_nonzero, d) + 1, (1,), generator=g))
        cols = torch.randperm(d, generator=g)[:k]
        f[i, cols] = torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
    return f


def exact_sums(x, y, degree):
    """Python integers N_xx, N_yy, N_xy with S = N / d^degree for gamma = 1 / d, coef = 1: sum of (dot + d)^degree"""
    d = x.shape[1]
    xi, yi = x.long(), y.long()
    gxx, gyy, gxy = (xi @ xi.T + d).tolist(), (yi @ yi.T + d).tolist(), (xi @ yi.T + d).tolist()
    m = len(gxx)
    nxx = sum(gxx[i][j] ** degree for i in range(m) for j in range(m) if i != j)
    nyy = sum(gyy[i][j] ** degree for i in range(m) for j in range(m) if i != j)
    nxy = sum(v ** degree for row in gxy for v in row)
    return nxx, nyy, nxy


@functools.lru_cache(maxsize=8)
def gaussian_like_features(n, d, seed):
    """non-negative fp32 rows with the rough statistics of pool3 features (post-ReLU means: |N(0.3, 0.3)| with a per-column scale);
    shared, do not modify"""
    g = torch.Generator().manual_seed(5000 + seed)
    return (0.3 + 0.3 * torch.randn(n, d, generator=g)).abs() * (0.5 + torch.rand(d, generator=g))


@functools.lru_cache(maxsize=2)
def synthetic_inception_state_dict(seed=0):
    """``fid_ref.synthetic_inception_state_dict`` with ``fc.weight`` = N(0, 1) sqrt(8 / 2048) of shape (1008, 2048): logits of a few units"""
    sd = dict(R.synthetic_inception_state_dict(seed))
    g = torch.Generator().manual_seed(7100 + seed)
    sd["fc.weight"] = torch.randn(CLASSES, 2048, generator=g) * math.sqrt(8.0 / 2048)
    return sd
