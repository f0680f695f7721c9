"""KID and the Inception score on the GPU (row N11) against tests/kid_ref.py: the MMD kernel on non-negative Gaussian-like
features under the fp64 summation bound, the Inception-score head on N(0, 3^2) logits within 1e-9 relative, and the two metric
classes over the FID tower: features bit-identical to ``InceptionV3FeaturesHIP``, KID against the restatement and against the fp32
tower (``KID_EMU_REL``: tests/test_kid_cpu.py measures it), one tower call feeding three metrics, torchmetrics' protocol.

Every figure is for the seeded weights of ``kid_ref.synthetic_inception_state_dict``: the real Inception checkpoint is not on
these machines.  Measured on an MI355X: see DESIGN.md section 9, N11."""
import functools
import math

import pytest
import torch

import fid_ref as R
import kid_ref as K

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=1)
def net():
    from mvd_amd.fid import InceptionV3FeaturesHIP
    return InceptionV3FeaturesHIP(K.synthetic_inception_state_dict(0))


@functools.lru_cache(maxsize=1)
def gpu_features():
    """pool3 features of fid_ref.test_images(0) from the GPU, (real, fake), on the device: one call each, shared; do not modify"""
    real, fake = R.test_images(0)
    return net()(real.cuda()), net()(fake.cuda())


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("m", [17, 130])
def test_kid_mmd_gaussian_like(m):
    """per subset |v - v_ref| <= 4 (m^2 + d) 2^-53 T (kid_ref.mmd_bound), default gamma / coef / degree, d = 2048, against the fp64
    restatement from the same fp32 features"""
    from mvd_amd import ops
    d, subsets = 2048, 3
    f_real, f_fake = K.gaussian_like_features(150, d, 0), K.gaussian_like_features(141, d, 1) * 1.1
    g = torch.Generator().manual_seed(m)
    draws = [(torch.randperm(150, generator=g)[:m], torch.randperm(141, generator=g)[:m]) for _ in range(subsets)]
    idx = torch.stack([torch.stack(p) for p in draws]).to(torch.int32)
    got, sums = ops.kid_mmd(f_real.cuda(), f_fake.cuda(), idx.cuda(), want_sums=True)
    want, scales = K.kid_scores(f_real, f_fake, subsets, m, draws=draws)
    worst = 0.0
    for s in range(subsets):
        err, bound = abs(float(got[s]) - float(want[s])), K.mmd_bound(m, d, scales[s])
        worst = max(worst, err / bound)
        print(f"kid_mmd m {m} subset {s}: {float(got[s]):.12e} vs {float(want[s]):.12e}, |diff| {err:.3e}, bound {bound:.3e}, T {scales[s]:.6g}")
    for s in range(subsets):
        assert math.isfinite(float(got[s])) and abs(float(got[s]) - float(want[s])) <= K.mmd_bound(m, d, scales[s])
        sxx, syy, sxy, _ = K.mmd_terms(f_real[draws[s][0]], f_fake[draws[s][1]])
        for a, b in zip(sums[s].tolist(), (sxx, syy, sxy)):
            # each side: d + 2 roundings in dot gamma + coef, tripled by the cube plus its two products, then at most m^2 additions;
            # the terms are non-negative, so the sum of the absolute terms is the sum itself
            assert abs(a - b) <= 2 * (3 * (d + 2) + 2 + m * m) * 2.0 ** -53 * abs(b)
    print(f"kid_mmd m {m}: worst |diff| / bound {worst:.3e}")


@pytest.mark.parametrize("splits", [1, 3, 10])
@pytest.mark.parametrize("n", [10, 25, 64, 130])
def test_inception_score_head(n, splits):
    """every chunk score within 1e-9 relative of the fp64 restatement (device against host exp / log), under a permutation that is
    not the identity; n = 25 with 10 splits has 9 chunks"""
    from mvd_amd import ops
    from mvd_amd.kid import chunk_bounds
    g = torch.Generator().manual_seed(1000 * n + splits)
    logits = 3.0 * torch.randn(n, K.CLASSES, generator=g)
    perm = torch.randperm(n, generator=g)
    assert not torch.equal(perm, torch.arange(n))
    got = ops.inception_score_chunks(logits.cuda(), perm.to(torch.int32).cuda(), splits)
    want = K.inception_score_chunks(logits, perm, splits)
    assert got.dtype == torch.float64 and got.shape == want.shape == (len(chunk_bounds(n, splits)),)
    rel = ((got.cpu() - want).abs() / want.abs()).max()
    print(f"inception score head n {n} splits {splits}: {want.shape[0]} chunk(s), worst relative difference {float(rel):.3e}")
    assert bool(((got.cpu() - want).abs() <= 1e-9 * want.abs()).all())
    assert torch.equal(got, ops.inception_score_chunks(logits.cuda(), perm.to(torch.int32).cuda(), splits))
    if 1 < len(want) < n:      # the permutation matters: the identity gives other chunks (chunks of one row all score exp(0))
        plain = K.inception_score_chunks(logits, torch.arange(n), splits)
        assert not bool(((plain - want).abs() <= 1e-9 * want.abs()).all())


# ------------------------------------------------------------------------------------------------ the metrics
M, SUBSETS = K.MEASURE["subset_size"], K.MEASURE["subsets"]


def kid(**kw):
    from mvd_amd.kid import KernelInceptionDistance
    kw.setdefault("inception", net())
    return KernelInceptionDistance(subsets=SUBSETS, subset_size=M, **kw)


def test_kid_features_are_the_towers():
    real, fake = R.test_images(0)
    m = kid()
    m.update(real.cuda(), real=True)
    m.update(fake[:1].cuda(), real=False)
    m.update(fake[1:].cuda(), real=False)
    g_real, g_fake = gpu_features()
    assert len(m.real_features) == 1 and len(m.fake_features) == 2 and m.real_features[0].dtype == torch.float32 and m.real_features[0].is_cuda
    assert torch.equal(m.real_features[0], g_real) and torch.equal(torch.cat(m.fake_features), g_fake)


def test_kid_fake_against_real():
    """a seeded compute() draws kid_ref's subsets; mean within the mean of the per-subset summation bounds of the restatement on the
    GPU's own features (the population std is 1-Lipschitz in the largest per-subset error; twice that for its own roundings), and
    within 2 KID_EMU_REL T of the fp32 tower's value"""
    g_real, g_fake = gpu_features()
    m = kid()
    m.update_features(g_real, real=True)
    m.update_features(g_fake, real=False)
    torch.manual_seed(0)
    mean, std = m.compute()
    assert mean.dim() == 0 and std.dim() == 0 and mean.is_cuda and mean.dtype == torch.float64 and std.dtype == torch.float64
    torch.manual_seed(0)
    draws = K.draw_subsets(4, 4, SUBSETS, M)
    own, scales = K.kid_scores(g_real, g_fake, SUBSETS, M, draws=draws)
    bounds = [K.mmd_bound(M, 2048, t) for t in scales]
    print(f"KID {float(mean):.12e} +- {float(std):.6e}; restatement on the GPU's features {float(own.mean()):.12e} +- {float(own.std(unbiased=False)):.6e}; "
          f"|diff| {abs(float(mean) - float(own.mean())):.3e}, bound {sum(bounds) / SUBSETS:.3e}")
    assert abs(float(mean) - float(own.mean())) <= sum(bounds) / SUBSETS
    assert abs(float(std) - float(own.std(unbiased=False))) <= 2 * max(bounds)
    want, scales32 = K.kid_scores(*R.reference_features(0, False), SUBSETS, M, draws=draws)
    t = sum(scales32) / SUBSETS
    print(f"fp32 tower {float(want.mean()):.9e}, T {t:.6f}: GPU off by {abs(float(mean) - float(want.mean())) / t:.3e} T (bound {2 * K.KID_EMU_REL:.1e} T)")
    assert abs(float(mean) - float(want.mean())) <= 2 * K.KID_EMU_REL * t
    torch.manual_seed(0)
    again = m.compute()
    assert torch.equal(again[0], mean) and torch.equal(again[1], std)


def test_kid_of_a_set_with_itself():
    """The unbiased estimate of a set against ITSELF is not zero: S_xy keeps the diagonal k(x_i, x_i) that S_xx drops.  What is zero
    to the summation bound: n copies of ONE image on both sides (every kernel value is the same).  With the same eight images on
    both sides and subset_size = 8, both subsets are the whole set: S_xx = S_yy, and the estimate equals the restatement."""
    real, fake = R.test_images(0)
    g_real, g_fake = gpu_features()
    one = kid()
    copies = real[:1].expand(4, -1, -1, -1).contiguous().cuda()
    one.update(copies, real=True)
    one.update(copies, real=False)
    mean, std = one.compute()
    t = K.mmd_terms(g_real[:1].expand(M, -1), g_real[:1].expand(M, -1))[3]
    print(f"KID of four copies of one image with themselves {float(mean):.3e} +- {float(std):.3e}, T {t:.6f}, bound {K.mmd_bound(M, 2048, t):.3e}")
    assert abs(float(mean)) <= K.mmd_bound(M, 2048, t) and float(std) <= 2 * K.mmd_bound(M, 2048, t)
    from mvd_amd.kid import KernelInceptionDistance
    both = torch.cat([g_real, g_fake])
    whole = KernelInceptionDistance(subsets=2, subset_size=8, inception=net())
    whole.update_features(both, real=True)
    whole.update_features(both, real=False)
    torch.manual_seed(3)
    mean, _ = whole.compute()
    torch.manual_seed(3)
    own, scales = K.kid_scores(both, both, 2, 8)
    assert abs(float(mean) - float(own.mean())) <= K.mmd_bound(8, 2048, max(scales))


def test_kid_protocol():
    from mvd_amd._lib import MvdError
    from mvd_amd.kid import KernelInceptionDistance
    real, fake = R.test_images(0)
    m = kid(reset_real_features=False).to("cuda")
    m.update(real.cuda(), real=True)
    m.update(fake.cuda(), real=False)
    torch.manual_seed(1)
    first = m.compute()
    kept = m.real_features[0]
    m.reset()      # reset_real_features=False: the real features stay
    assert m.fake_features == [] and len(m.real_features) == 1 and m.real_features[0] is kept
    with pytest.raises(ValueError, match="should be smaller than the number of samples"):
        m.compute()
    m(fake.cuda(), real=False)
    torch.manual_seed(1)
    assert torch.equal(m.compute()[0], first[0])
    full = kid()
    full.update(real.cuda(), real=True)
    full.reset()
    assert full.real_features == [] and full.fake_features == []
    # errors come before any launch
    big = KernelInceptionDistance(subsets=2, subset_size=5, inception=net())
    big.update_features(gpu_features()[0], real=True)
    big.update_features(torch.cat(gpu_features()), real=False)
    with pytest.raises(ValueError, match="should be smaller than the number of samples"):
        big.compute()
    with pytest.raises(MvdError, match="GPU only"):
        full.update(real, real=True)
    with pytest.raises(MvdError, match="GPU only"):
        full.update_features(gpu_features()[0].cpu(), real=True)
    with pytest.raises(MvdError, match="uint8"):
        full.update(real.float().cuda(), real=True)
    with pytest.raises(MvdError, match="fp32"):
        full.update_features(gpu_features()[0].double(), real=True)
    with pytest.raises(MvdError, match="floating-point"):
        kid(normalize=True).update(real.cuda(), real=True)
    as_float = kid(normalize=True)
    as_float.update(real.float().cuda() / 255.0, real=True)
    assert torch.equal(as_float.real_features[0], gpu_features()[0])


def test_inception_score_through_the_class():
    from mvd_amd import ops
    from mvd_amd._lib import MvdError
    from mvd_amd.kid import InceptionScore
    real, fake = R.test_images(0)
    imgs = torch.cat([real, fake]).cuda()
    feats = torch.cat(gpu_features())
    s = InceptionScore(splits=3, inception=net())
    s.update(imgs[:5])
    s(imgs[5:])
    logits = torch.cat(s.features)
    assert logits.shape == (8, K.CLASSES) and logits.dtype == torch.float32
    w = K.synthetic_inception_state_dict(0)["fc.weight"]
    assert torch.equal(logits, ops.fc_logits(feats, w.cuda())) and torch.equal(logits, net().logits(feats))
    ref = feats.cpu().double() @ w.double().T
    assert float((logits.cpu().double() - ref).abs().max()) <= 2048 * 2.0 ** -24 * float((feats.cpu().abs().double() @ w.abs().double().T).max())
    torch.manual_seed(2)
    mean, std = s.compute()
    torch.manual_seed(2)
    want = K.inception_score_chunks(logits, torch.randperm(8), 3)
    print(f"Inception score {float(mean):.12f} +- {float(std):.6e}; restatement on the GPU's logits {float(want.mean()):.12f} +- {float(want.std()):.6e}")
    assert mean.dim() == 0 and mean.is_cuda and mean.dtype == torch.float64
    assert abs(float(mean) - float(want.mean())) <= 1e-9 * float(want.mean())
    assert abs(float(std) - float(want.std())) <= 2e-9 * float(want.max())      # torch.std (unbiased), 1-Lipschitz up to sqrt(3 / 2)
    single = InceptionScore(splits=1, inception=net())
    single.update_features(feats)
    one_mean, one_std = single.compute()
    assert math.isfinite(float(one_mean)) and math.isnan(float(one_std))      # torch.std of one chunk
    s.reset()
    assert s.features == []
    with pytest.raises(MvdError, match="GPU only"):
        s.update(real)
    bare = {k: v for k, v in K.synthetic_inception_state_dict(0).items() if k != "fc.weight"}
    with pytest.raises(MvdError, match="no 'fc.weight'"):
        InceptionScore(weights=bare)


def test_one_tower_feeds_three_metrics():
    """update_features on FID, KID and the Inception score from ONE tower call per batch == three separate update calls, bit for bit"""
    from mvd_amd.fid import FrechetInceptionDistance
    from mvd_amd.kid import InceptionScore, KernelInceptionDistance
    real, fake = (t.cuda() for t in R.test_images(0))
    sd = K.synthetic_inception_state_dict(0)
    tower = net()
    shared = (FrechetInceptionDistance(inception=tower), KernelInceptionDistance(subsets=SUBSETS, subset_size=M, inception=tower),
              InceptionScore(splits=2, inception=tower))
    apart = (FrechetInceptionDistance(weights=sd), KernelInceptionDistance(subsets=SUBSETS, subset_size=M, weights=sd), InceptionScore(splits=2, weights=sd))
    for imgs, is_real in ((real, True), (fake[:3], False), (fake[3:], False)):
        pool3 = tower(imgs)
        shared[0].update_features(pool3, real=is_real)
        shared[1].update_features(pool3, real=is_real)
        apart[0].update(imgs, real=is_real)
        apart[1].update(imgs, real=is_real)
        if not is_real:
            shared[2].update_features(pool3)
            apart[2].update(imgs)
    for name in FrechetInceptionDistance.STATE:
        assert torch.equal(getattr(shared[0], name), getattr(apart[0], name)), name
    assert float(shared[0].compute()) == float(apart[0].compute())
    results = []
    for group in (shared, apart):
        torch.manual_seed(4)
        results.append((group[1].compute(), group[2].compute()))
    for a, b in zip(results[0], results[1]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
