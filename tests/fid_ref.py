"""FID's feature extractor (the FID variant of Inception-v3 up to pool3) and torchmetrics' ``FrechetInceptionDistance`` arithmetic,
restated with ``F.conv2d`` / ``F.relu`` / ``F.avg_pool2d(count_include_pad=False)`` / ``F.max_pool2d`` only -- neither torchmetrics
nor torch-fidelity is installed where this project runs, so this file is what the GPU path is compared with;
tests/test_fid_cpu.py checks it against those packages where they import.

The tower walks ``mvd_amd.packing.INCEPTION_FID_LAYERS``, the one layer table of the project.  In front of it: the TF1-legacy
bilinear resize to 299 x 299 in fp32 (src = dst * float32(in / out), i0 = floor, i1 = min(i0 + 1, in - 1),
top = tl + (tr - tl) wx, out = top + (bot - top) wy, every operation rounded on its own), then (v - 128) / 128.  Both towers use the
folded weights (BatchNorm eps 1e-3 folded in fp32) AFTER their rounding to bf16, the folded biases in fp32.

``emulate_bf16`` rounds at the storage points of the GPU path: the normalised input, every post-ReLU map and every pooled map,
but not Mixed_7c (fp32 there and here).  The distance between the emulation and the plain fp32 tower is the error the number
format alone causes; the GPU tests bound the kernels by twice that (``FEAT_EMU_REL``, ``FID_EMU_REL``: measured by
tests/test_fid_cpu.py::test_emulation_error_constants, which keeps them between the measured maximum and twice it).

Plain helper module (like lpips_ref.py), no fixtures."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from mvd_amd import packing as P

SIZE = P.FID_INPUT_SIZE
# maxima over seeds 0-2 of tests/test_fid_cpu.py::test_emulation_error_constants (four real and four fake images of 64 x 64):
# per-image rel-L2 distance of the bf16 emulation's pool3 features to the fp32 tower's, and |FID_emu - FID_fp32| / FID_fp32
FEAT_EMU_REL = 1.0e-3      # measured maximum 9.67e-4
FID_EMU_REL = 2.3e-3       # measured maximum 2.20e-3 (seed 1; FID 0.62 - 2.66 over the seeds)
MEASURE_SEEDS = (0, 1, 2)


# ------------------------------------------------------------------------------------------------ weights
@functools.lru_cache(maxsize=2)
def synthetic_inception_state_dict(seed=0):
    """He-initialised convolutions (std sqrt(2 / (kh kw cin))), BatchNorm gamma = 1 + 0.1 N, beta and running mean 0.05 N,
    running variance 1 + 0.1 |N|, under torch-fidelity's keys; ``fc.*`` and ``num_batches_tracked`` are there to be ignored"""
    g = torch.Generator().manual_seed(7000 + seed)
    sd = {}
    for e in P.INCEPTION_FID_CONVS:
        name, cin, cout, kh, kw = e[1], e[5], e[6], e[7], e[8]
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (kh * kw * cin))
        sd[f"{name}.bn.weight"] = 1.0 + 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.05 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.05 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 1.0 + 0.1 * torch.randn(cout, generator=g).abs()
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = torch.zeros(1008, 2048)
    sd["fc.bias"] = torch.zeros(1008)
    return sd


@functools.lru_cache(maxsize=2)
def folded(seed=0):
    """name -> (folded weight, bf16 values as fp32; folded bias fp32): what both towers and the kernels compute with"""
    return {n: (w.float(), b) for n, (w, b) in P.fold_inception_fid(synthetic_inception_state_dict(seed)).items()}


# ------------------------------------------------------------------------------------------------ front end
def quantise(x):
    """torchmetrics' normalize=True: (x * 255).byte() for x in [0, 1]; outside it the GPU path clamps (``.byte()`` is undefined there)"""
    return torch.trunc(x.float().clamp(0.0, 1.0) * 255.0)


def resize_tf1(v, size=SIZE):
    """v (B, 3, H, W) fp32 -> (B, 3, size, size) fp32, one rounding per written operation"""
    v = v.float()
    H, W = v.shape[2:]
    sh, sw = torch.tensor(np.float32(H / size)), torch.tensor(np.float32(W / size))
    ys, xs = torch.arange(size, dtype=torch.float32) * sh, torch.arange(size, dtype=torch.float32) * sw
    y0f, x0f = torch.floor(ys), torch.floor(xs)
    wy, wx = (ys - y0f).view(1, 1, size, 1), (xs - x0f).view(1, 1, 1, size)
    y0, x0 = y0f.long().clamp(max=H - 1), x0f.long().clamp(max=W - 1)
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    tl, tr = v[:, :, y0][:, :, :, x0], v[:, :, y0][:, :, :, x1]
    bl, br = v[:, :, y1][:, :, :, x0], v[:, :, y1][:, :, :, x1]
    top = tl + (tr - tl) * wx
    bot = bl + (br - bl) * wx
    return top + (bot - top) * wy


def front_end(images):
    """uint8, or floating point in [0, 1] -> the normalised (B, 3, 299, 299) fp32 map"""
    v = images.float() if images.dtype == torch.uint8 else quantise(images)
    return (resize_tf1(v) - 128.0) / 128.0


# ------------------------------------------------------------------------------------------------ tower
def tower(x, weights, emulate_bf16=False, layers=P.INCEPTION_FID_LAYERS, keep=None):
    """x: the front end's output (B, 3, h, w) -> the fp32 map of ``FID_FEATURE_BUFFER`` (``keep``: a dict that receives every buffer)"""
    r = (lambda t: t.to(torch.bfloat16).float()) if emulate_bf16 else (lambda t: t)
    ch = P.fid_buffer_channels(layers)
    bufs = {"img": r(x)}
    for e in layers:
        src = bufs[e[2]]
        if e[0] == "conv":
            _, name, _, dst, c_off, cin, cout, kh, kw, stride, ph, pw = e
            w, b = weights[name]
            y = F.relu(F.conv2d(src, w, b, stride=stride, padding=(ph, pw)))
        else:
            _, mode, _, dst, c_off, cout = e
            y = (F.avg_pool2d(src, 3, 1, 1, count_include_pad=False) if mode == "avg" else F.max_pool2d(src, 3, 1, 1) if mode == "max1"
                 else F.max_pool2d(src, 3, 2))
        if dst != P.FID_FEATURE_BUFFER:
            y = r(y)
        if dst not in bufs:
            bufs[dst] = torch.zeros(y.shape[0], ch[dst], y.shape[2], y.shape[3])
        bufs[dst][:, c_off:c_off + cout] = y
    if keep is not None:
        keep.update(bufs)
    return bufs[P.FID_FEATURE_BUFFER]


@torch.no_grad()
def features(images, seed=0, emulate_bf16=False):
    """pool3 features (B, 2048) fp32 of uint8 / [0, 1] images under the synthetic weights of ``seed``"""
    out = []
    for i in range(images.shape[0]):      # one image at a time: the memory of the 147 x 147 maps
        out.append(tower(front_end(images[i:i + 1]), folded(seed), emulate_bf16).mean((2, 3)))
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------ torchmetrics' update / compute, fp64
def new_state(d=2048):
    return dict(sum=torch.zeros(d, dtype=torch.float64), cov_sum=torch.zeros(d, d, dtype=torch.float64), n=0)


def tm_update(state, feats):
    """FrechetInceptionDistance.update after the network: features.double(), sum += f.sum(0), cov_sum += f^T f, n += rows"""
    f = feats.detach().cpu().double()
    state["sum"] += f.sum(0)
    state["cov_sum"] += f.t().mm(f)
    state["n"] += f.shape[0]
    return state


def tm_statistics(state):
    """compute()'s first half: mean = sum / n, cov = (cov_sum - n mean mean^T) / (n - 1)"""
    n = state["n"]
    mean = (state["sum"] / n).unsqueeze(0)
    cov = (state["cov_sum"] - n * mean.t().mm(mean)) / (n - 1)
    return mean.squeeze(0), cov


def tm_compute_fid(mu1, sigma1, mu2, sigma2):
    """torchmetrics' ``_compute_fid``, literally: the trace term from the eigenvalues of the (unsymmetric) product"""
    a = (mu1 - mu2).square().sum(dim=-1)
    b = sigma1.trace() + sigma2.trace()
    c = torch.linalg.eigvals(sigma1 @ sigma2).sqrt().real.sum(dim=-1)
    return a + b - 2 * c


def trace_sqrt_from_features(f1, f2):
    """tr sqrt(S1 S2) for sample covariances of FEW samples, from the features themselves: with A_k the centred (n_k, d) feature
    matrices, S_k = A_k^T A_k / (n_k - 1), and the non-zero eigenvalues of S1 S2 are those of (A1 A2^T)(A1 A2^T)^T /
    ((n1 - 1)(n2 - 1)): the trace term is the nuclear norm of the n1 x n2 matrix A1 A2^T, scaled.  No d x d eigenproblem, no
    square root of a rounding-noise eigenvalue: this form's own error is a few ulps, which is what a 1e-9 comparison needs when
    the covariances have rank n - 1 << d (the literal ``eigvals`` form gives 2048 - rank eigenvalues of size eps |S|^2, whose
    square roots add up to about 1e-5 of the result)."""
    a1 = f1.double() - f1.double().mean(0, keepdim=True)
    a2 = f2.double() - f2.double().mean(0, keepdim=True)
    sv = torch.linalg.svdvals(a1 @ a2.t())
    return sv.sum() / math.sqrt((f1.shape[0] - 1) * (f2.shape[0] - 1))


def fid_of_features(f_real, f_fake):
    """torchmetrics' update / compute in fp64 over two feature sets (one update each): the means and covariances from the sums
    as ``tm_statistics`` forms them, the trace term by ``trace_sqrt_from_features`` -> (fid, tr S_real + tr S_fake)"""
    s1, s2 = tm_update(new_state(f_real.shape[1]), f_real), tm_update(new_state(f_fake.shape[1]), f_fake)
    mu1, c1 = tm_statistics(s1)
    mu2, c2 = tm_statistics(s2)
    tr = c1.trace() + c2.trace()
    fid = (mu1 - mu2).square().sum() + tr - 2.0 * trace_sqrt_from_features(f_real.detach().cpu(), f_fake.detach().cpu())
    return float(fid), float(tr)


# ------------------------------------------------------------------------------------------------ the test images
def _smooth(g, n, size, cells=6):
    low = torch.rand(n, 3, cells, cells, generator=g)
    return F.interpolate(low, size=(size, size), mode="bilinear", align_corners=True)


@functools.lru_cache(maxsize=8)
def test_images(seed=0, n=4, size=64):
    """(real, fake) uint8 (n, 3, size, size): real = a smooth random field plus noise; fake = the same law (other draws), shifted in
    brightness and blurred, so the FID of the pair is well away from 0"""
    g = torch.Generator().manual_seed(9000 + seed)
    real = _smooth(g, n, size) * 0.8 + 0.1 + 0.08 * torch.randn(n, 3, size, size, generator=g)
    fake = _smooth(g, n, size) * 0.8 + 0.1 + 0.08 * torch.randn(n, 3, size, size, generator=g)
    fake = F.avg_pool2d(F.pad(fake, (1, 1, 1, 1), mode="replicate"), 3, 1) + 0.08
    to_u8 = lambda t: (t.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)      # noqa: E731
    return to_u8(real), to_u8(fake)


test_images.__test__ = False      # (a helper, not a test: pytest collects test_* names of imported modules only from test files)


@functools.lru_cache(maxsize=8)
def reference_features(seed=0, emulate_bf16=False, n=4, size=64):
    """(real, fake) pool3 features of ``test_images`` -- computed once per process and shared; do not modify"""
    real, fake = test_images(seed, n, size)
    return features(real, seed, emulate_bf16), features(fake, seed, emulate_bf16)
