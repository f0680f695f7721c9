"""Precision / recall and density / coverage on the GPU (row N12) against tests/prdc_ref.py.

Operators: non-negative low-rank features ``|z A|`` (z n x 8, A 8 x 2048), the fake side scaled 1.1 and shifted 0.2 -- all four
metrics are well inside (0, 1) there (plain Gaussian rows at d = 2048 give a degenerate precision near 0.008).  Each case FIRST
asserts, on the restatement alone, that no predicate entry is a near-tie: every |D2 - radius| exceeds twice the rounding bound
4 d 2^-53 (|q|^2 + |r|^2) (the Gram-form error: dot product and two norms, each gamma_d, with a factor 2 of slack).  Then the counts
must EQUAL the restatement's and ``radii_sq`` lie within the bound.  A near-tie would be a failed precondition, not a skipped case.

Classes, with the seeded tower weights of ``kid_ref.synthetic_inception_state_dict``: ``update`` stores the tower's features bit for
bit, ``compute()`` equals the restatement on those features, one tower call feeds FID, KID and the two metrics, the identities of
tests/test_prdc_cpu.py hold, ``reset`` works and ``compute()`` does not synchronise."""
import functools

import pytest
import torch

import fid_ref as R
import kid_ref as K
import prdc_ref as P

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
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n", [130, 257])
def test_operators_on_lowrank_features(n, seed):
    from mvd_amd import ops
    real, fake = P.lowrank_features(n, 2 * seed), P.lowrank_features(n - 7, 2 * seed + 1, 1.1, 0.2)
    rd, fd = real.cuda(), fake.cuda()
    d_fr = P.d2(fake, real)
    for k, closed in ((3, True), (5, False)):
        for q, r, qd_, rd_, dist in ((fake, real, fd, rd, d_fr), (real, fake, rd, fd, d_fr.T)):
            want_radii = P.radii(r, k)
            margin = P.min_margin(q, r, want_radii)
            print(f"n {n} seed {seed} k {k} {'closed' if closed else 'open'}: smallest |D2 - radius| = {margin:.3e} bounds")
            assert margin > 2.0, "precondition: a predicate entry is a near-tie"
            radii = ops.knn_radii(rd_, k)
            bound = P.gram_bound(r, r).max(dim=1).values      # an order statistic moves by at most the largest move of an entry
            err = (radii.cpu() - want_radii).abs()
            print(f"    radii_sq: worst |diff| / bound {float((err / bound).max()):.3e}")
            assert bool((err <= bound).all())
            want_q, want_r = P.counts(dist, want_radii, closed)
            hq, hr = ops.manifold_counts(qd_, rd_, radii, closed)
            assert torch.equal(hq.cpu(), want_q) and torch.equal(hr.cpu(), want_r)
            assert 0 < int(want_q.sum()) < dist.numel()
            again_q, again_r = ops.manifold_counts(qd_, rd_, ops.knn_radii(rd_, k), closed)
            assert torch.equal(again_q, hq) and torch.equal(again_r, hr)


def test_module_functions():
    from mvd_amd import ops, prdc
    real, fake = P.lowrank_features(130, 0).cuda(), P.lowrank_features(123, 1, 1.1, 0.2).cuda()
    radii = prdc.knn_radii(real, 3)
    assert torch.equal(radii, ops.knn_radii(real, 3))
    hq, hr = prdc.manifold_counts(fake, real, radii, True)
    want = ops.manifold_counts(fake, real, radii, True)
    assert torch.equal(hq, want[0]) and torch.equal(hr, want[1])
    with pytest.raises(ValueError, match="at least 4 samples"):
        prdc.knn_radii(real[:3], 3)
    with pytest.raises(ValueError, match="k must be"):
        prdc.knn_radii(real, 16)


# ------------------------------------------------------------------------------------------------ the metrics
def metrics(**kw):
    """k = 2 on both: the tower cases have four real and four fake images"""
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    kw.setdefault("inception", net())
    return PrecisionRecall(neighborhood=2, **kw), DensityCoverage(nearest_k=2, **kw)


def assert_result(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dim() == 0 and g.is_cuda and g.dtype == torch.float64
        assert float(g) == w, (float(g), w)


def test_features_are_the_towers():
    real, fake = R.test_images(0)
    g_real, g_fake = gpu_features()
    for m in metrics():
        m.update(real.cuda(), real=True)
        m.update(fake[:1].cuda(), real=False)
        m(fake[1:].cuda(), real=False)
        assert len(m.real_features) == 1 and len(m.fake_features) == 2 and m.real_features[0].dtype == torch.float32 and m.real_features[0].is_cuda
        assert torch.equal(m.real_features[0], g_real) and torch.equal(torch.cat(m.fake_features), g_fake)
    as_float = metrics(normalize=True)[0]
    as_float.update(real.float().cuda() / 255.0, real=True)
    assert torch.equal(as_float.real_features[0], g_real)


def test_compute_equals_the_restatement():
    """the four real images and one fake image as the real side, the other three fake images as the fake side (the plain four
    against four are disjoint clusters: all zeros), k = 2: the metrics are strictly between 0 and 1"""
    from mvd_amd.prdc import PrecisionRecall
    g_real, g_fake = gpu_features()
    side_r, side_f = torch.cat([g_real, g_fake[:1]]), g_fake[1:].contiguous()
    for r, q in ((side_r, side_f), (side_f, side_r)):
        assert P.min_margin(q, r, P.radii(r, 2)) > 2.0, "precondition: a predicate entry is a near-tie"
    pr, dc = metrics()
    for m in (pr, dc):
        m.update_features(g_real, real=True)
        m.update_features(g_fake[:1], real=True)
        m.update_features(g_fake[1:3], real=False)
        m.update_features(g_fake[3:], real=False)
    want_pr, want_dc = P.precision_recall(side_r, side_f, 2), P.density_coverage(side_r, side_f, 2)
    print(f"precision, recall, f_score {want_pr}; density, coverage {want_dc}")
    assert 0.0 < want_pr[1] < 1.0 and 0.0 < want_pr[2] < 1.0 and 0.0 < want_dc[0] < 1.0 and 0.0 < want_dc[1] < 1.0
    assert_result(pr.compute(), want_pr)
    assert_result(dc.compute(), want_dc)
    open_pr = PrecisionRecall(neighborhood=2, strict=True, inception=net())
    open_pr.update_features(side_r, real=True)
    open_pr.update_features(side_f, real=False)
    assert_result(open_pr.compute(), P.precision_recall(side_r, side_f, 2, strict=True))
    again = pr.compute()
    assert all(torch.equal(a, b) for a, b in zip(again, pr.compute()))


def test_one_tower_feeds_four_metrics():
    """update_features on FID, KID, PrecisionRecall and DensityCoverage from ONE tower call per batch == four separate update calls,
    bit for bit"""
    from mvd_amd.fid import FrechetInceptionDistance
    from mvd_amd.kid import KernelInceptionDistance
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    real, fake = (t.cuda() for t in R.test_images(0))
    sd = K.synthetic_inception_state_dict(0)
    tower = net()
    m, subsets = K.MEASURE["subset_size"], K.MEASURE["subsets"]
    shared = (FrechetInceptionDistance(inception=tower), KernelInceptionDistance(subsets=subsets, subset_size=m, inception=tower),
              PrecisionRecall(neighborhood=2, inception=tower), DensityCoverage(nearest_k=2, inception=tower))
    apart = (FrechetInceptionDistance(weights=sd), KernelInceptionDistance(subsets=subsets, subset_size=m, weights=sd),
             PrecisionRecall(neighborhood=2, weights=sd), DensityCoverage(nearest_k=2, weights=sd))
    for imgs, is_real in ((real, True), (fake[:3], False), (fake[3:], False)):
        pool3 = tower(imgs)
        for a, b in zip(shared, apart):
            a.update_features(pool3, real=is_real)
            b.update(imgs, real=is_real)
    for name in FrechetInceptionDistance.STATE:
        assert torch.equal(getattr(shared[0], name), getattr(apart[0], name)), name
    assert float(shared[0].compute()) == float(apart[0].compute())
    for a, b in zip(shared[1:], apart[1:]):
        for side in ("real_features", "fake_features"):
            assert torch.equal(torch.cat(getattr(a, side)), torch.cat(getattr(b, side)))
        torch.manual_seed(4)
        ra = a.compute()
        torch.manual_seed(4)
        rb = b.compute()
        assert len(ra) == len(rb) and all(torch.equal(x, y) for x, y in zip(ra, rb))


@pytest.mark.parametrize("n", [130, 257])
def test_identities(n):
    """the same set on both sides (rows in general position: tests/test_prdc_cpu.py::test_identities) gives precision = recall =
    f_score = coverage = 1 and density = 1 EXACTLY; two sets 100 apart give all zeros"""
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    f = P.lowrank_features(n, 0)
    assert P.min_margin(f, f, P.radii(f, 5)) == 0.0      # the set's own radii are entries of its own D2 ...
    fd = f.cuda()
    pr, dc = PrecisionRecall(inception=net()), DensityCoverage(inception=net())
    for m in (pr, dc):
        m.update_features(fd, real=True)
        m.update_features(fd, real=False)
    # ... so the open comparison of density relies on the kernels computing D2(f_i, f_j) to the same bits in knn_radii and in
    # manifold_counts: both run gram_tile on the same rows in the same order
    assert_result(pr.compute(), (1.0, 1.0, 1.0))
    assert_result(dc.compute(), (1.0, 1.0))
    far = (f + 100.0).cuda()
    for m in (pr, dc):
        m.reset()
        m.update_features(fd, real=True)
        m.update_features(far, real=False)
    assert_result(pr.compute(), (0.0, 0.0, 0.0))
    assert_result(dc.compute(), (0.0, 0.0))


def test_protocol():
    from mvd_amd._lib import MvdError
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    g_real, g_fake = gpu_features()
    for cls, kw in ((PrecisionRecall, dict(neighborhood=2)), (DensityCoverage, dict(nearest_k=2))):
        m = cls(reset_real_features=False, inception=net(), **kw).to("cuda")
        m.update_features(g_real, real=True)
        m.update_features(g_fake, real=False)
        first = m.compute()
        kept = m.real_features[0]
        m.reset()      # reset_real_features=False: the real features stay
        assert m.fake_features == [] and len(m.real_features) == 1 and m.real_features[0] is kept
        with pytest.raises(ValueError, match="fake samples"):
            m.compute()
        m.update_features(g_fake, real=False)
        assert all(torch.equal(a, b) for a, b in zip(m.compute(), first))
        full = cls(inception=net(), **kw)
        full.update_features(g_real, real=True)
        full.reset()
        assert full.real_features == [] and full.fake_features == []
        # errors come before any launch
        few = cls(inception=net())      # the default k needs more than four samples
        few.update_features(g_real[:3], real=True)
        few.update_features(g_fake, real=False)
        with pytest.raises(ValueError, match="real samples, got 3"):
            few.compute()
        with pytest.raises(MvdError, match="GPU only"):
            full.update(R.test_images(0)[0], real=True)
        with pytest.raises(MvdError, match="GPU only"):
            full.update_features(g_real.cpu(), real=True)
        with pytest.raises(MvdError, match="uint8"):
            full.update(R.test_images(0)[0].float().cuda(), real=True)
        with pytest.raises(MvdError, match="fp32"):
            full.update_features(g_real.double(), real=True)


def test_compute_does_not_synchronise():
    real, fake = P.lowrank_features(130, 0).cuda(), P.lowrank_features(123, 1, 1.1, 0.2).cuda()
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    pr, dc = PrecisionRecall(inception=net()), DensityCoverage(inception=net())
    for m in (pr, dc):
        m.update_features(real, real=True)
        m.update_features(fake, real=False)
    warm = pr.compute(), dc.compute()      # the allocator has its blocks, the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = pr.compute(), dc.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(warm, got):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert_result(got[0], P.precision_recall(real, fake, 3))
    assert_result(got[1], P.density_coverage(real, fake, 5))
