"""Precision / recall and density / coverage (row N12) without a GPU: the restatement of tests/prdc_ref.py against its exact integer
path, against the packages where they import and on two identities; the host logic of mvd_amd/prdc.py (constructor and compute
errors, tower sharing); the exported symbols and their host-side argument checks; and the fault sensitivity of the integer inputs
the exact GPU tests use, on a CPU emulation of the kernels' tiling."""
import ctypes as C

import pytest
import torch

import kid_ref as K
import prdc_ref as P
from mvd_amd import _lib as L
from mvd_amd._lib import MvdError


# ------------------------------------------------------------------------------------------------ restatement == integer path
@pytest.mark.parametrize("n,m,d", [(67, 61, 64), (130, 141, 64), (130, 150, 2048)])
def test_restatement_equals_integer_path(n, m, d):
    """on features over {-1, 0, 1} every norm, dot product and D2 is an integer below 2^13: the fp64 Gram form is exact, so the
    restatement must equal int64 ((a - b)^2).sum() entry by entry, and so must everything derived from it"""
    real, fake = P.ternary_features(n, d, 0), P.ternary_features(m, d, 1)
    assert 4 * d < 2 ** 13 + 1 and set(real.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for a, b in ((real, real), (fake, real), (real, fake)):
        assert torch.equal(P.d2(a, b), P.d2_int(a, b).double())
    for k in (1, 3, 5, 15):
        assert torch.equal(P.radii(real, k), P.radii(real, k, P.d2_int(real, real)).double())
        assert torch.equal(P.knn_list(real, k), P.knn_list(real, k, P.d2_int(real, real)).double())
    for strict in (False, True):
        assert P.precision_recall(real, fake, 3, strict) == P.precision_recall_int(real, fake, 3, strict)
    assert P.density_coverage(real, fake, 5) == P.density_coverage_int(real, fake, 5)
    for closed in (False, True):
        r = P.radii(real, 3)
        hq, hr = P.counts(P.d2(fake, real), r, closed)
        hq_i, hr_i = P.counts(P.d2_int(fake, real), P.radii(real, 3, P.d2_int(real, real)), closed)
        assert torch.equal(hq, hq_i) and torch.equal(hr, hr_i)


def test_integer_inputs_are_full_of_ties():
    """what makes the exact GPU tests sharp: entries ON the threshold (closed and open differ), rows whose k-th and (k + 1)-th values
    are equal (ties inside the list) and rows where they differ (k-th for (k + 1)-th shows)"""
    for n, d in ((67, 64), (130, 64), (130, 2048), (257, 2048)):
        dist, k = P.ternary_d2(n, d, 0), 3
        lst = P.knn_list(None, k, dist)
        on_threshold = int((dist == lst[:, k][None]).sum())
        tie, differ = int((lst[:, k] == lst[:, k - 1]).sum()), int((lst[:, k] != lst[:, k - 1]).sum())
        hq_closed, _ = P.counts(dist, lst[:, k], True)
        hq_open, _ = P.counts(dist, lst[:, k], False)
        print(f"n {n} d {d}: {on_threshold} entries on the threshold, {tie} rows with a tie at the k-th position, {differ} without; "
              f"hit totals closed / open {int(hq_closed.sum())} / {int(hq_open.sum())}")
        assert on_threshold > 0 and tie > 0 and differ > 0 and int(hq_closed.sum()) > int(hq_open.sum())


# ------------------------------------------------------------------------------------------------ against the packages
def test_precision_recall_against_torch_fidelity():
    tf = pytest.importorskip("torch_fidelity.metric_prc")
    real, fake = P.lowrank_features(60, 0, d=256), P.lowrank_features(50, 1, 1.1, 0.2, d=256)
    want = tf.prc_features_to_metric(real.double(), fake.double(), neighborhood=3)
    p, r, f = P.precision_recall(real, fake, 3)
    assert (p, r) == (float(want["precision"]), float(want["recall"])) and abs(f - float(want["f_score"])) <= 1e-12


def test_density_coverage_against_prdc():
    prdc = pytest.importorskip("prdc")
    real, fake = P.lowrank_features(60, 0, d=256), P.lowrank_features(50, 1, 1.1, 0.2, d=256)
    want = prdc.compute_prdc(real.double().numpy(), fake.double().numpy(), nearest_k=5)
    dens, cov = P.density_coverage(real, fake, 5)
    assert abs(dens - float(want["density"])) <= 1e-12 and cov == float(want["coverage"])
    p, r, _ = P.precision_recall(real, fake, 5, strict=True)
    assert (p, r) == (float(want["precision"]), float(want["recall"]))


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("n", [130, 257])
def test_identities(n):
    """the same set on both sides, rows in general position (no two D2 of a row equal): every sample lies within its own radius
    (D2 = 0 < radius), so precision = recall = coverage = 1, and row i lies strictly inside exactly the k balls whose (k + 1)-list
    holds it below the radius -- summed over the set that is k n, so density = 1 EXACTLY.  Two sets 100 apart: all zeros."""
    f = P.lowrank_features(n, 0)
    lst = P.knn_list(f, 5)
    assert bool((lst[:, 1:] != lst[:, :-1]).all()), "rows are not in general position"
    assert P.precision_recall(f, f, 3) == (1.0, 1.0, 1.0) and P.precision_recall(f, f, 3, strict=True) == (1.0, 1.0, 1.0)
    assert P.density_coverage(f, f, 5) == (1.0, 1.0)
    far = f + 100.0
    assert float(P.d2(f, far).min()) > float(P.radii(f, 5).max()) and float(P.d2(f, far).min()) > float(P.radii(far, 5).max())
    assert P.precision_recall(f, far, 3) == (0.0, 0.0, 0.0)
    assert P.density_coverage(f, far, 5) == (0.0, 0.0)


def test_lowrank_inputs_are_not_degenerate():
    """the GPU test's inputs: all four metrics well inside (0, 1), and no predicate entry near its threshold"""
    for n in (130, 257):
        real, fake = P.lowrank_features(n, 0), P.lowrank_features(n, 1, 1.1, 0.2)
        vals = P.precision_recall(real, fake, 3)[:2] + P.density_coverage(real, fake, 5)
        print(f"n {n}: precision, recall, density, coverage = {vals}")
        assert all(0.5 < v < 0.99 for v in vals)
        assert P.min_margin(fake, real, P.radii(real, 3)) > 2 and P.min_margin(real, fake, P.radii(fake, 3)) > 2


# ------------------------------------------------------------------------------------------------ host logic
def test_constructor_and_compute_errors():
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall, knn_radii, manifold_counts
    sd = K.synthetic_inception_state_dict(0)
    for cls in (PrecisionRecall, DensityCoverage):
        for feature in (64, 192, 768, "2048", 2048.0, True):
            with pytest.raises(ValueError, match="only the 2048"):
                cls(feature=feature, weights=sd)
        for kw, msg in ((dict(reset_real_features=1), "`reset_real_features`"), (dict(normalize=0), "`normalize`"), (dict(inception="net"), "InceptionV3FeaturesHIP")):
            with pytest.raises(ValueError, match=msg):
                cls(weights=sd, **kw)
    for bad in (0, 16, 3.0, True, None):
        with pytest.raises(ValueError, match="`neighborhood`"):
            PrecisionRecall(weights=sd, neighborhood=bad)
        with pytest.raises(ValueError, match="`nearest_k`"):
            DensityCoverage(weights=sd, nearest_k=bad)
    with pytest.raises(ValueError, match="`strict`"):
        PrecisionRecall(weights=sd, strict=1)
    pr = PrecisionRecall(weights=sd, device="cpu")
    dc = DensityCoverage(weights=sd, device="cpu")
    assert pr.neighborhood == 3 and pr.strict is False and dc.nearest_k == 5
    assert pr.real_features == [] and pr.fake_features == [] and dc.real_features == [] and dc.fake_features == []
    # too few samples: a ValueError before anything is launched (no GPU here: a launch would raise something else).  The state is
    # set directly: update_features takes device tensors only
    f = torch.zeros(4, 2048)
    with pytest.raises(ValueError, match="at least 4 real samples, got 0"):
        pr.compute()
    pr.real_features, pr.fake_features = [f], [f[:3]]
    with pytest.raises(ValueError, match="at least 4 fake samples, got 3"):
        pr.compute()
    pr.real_features, pr.fake_features = [f[:2], f[:1]], [f]
    with pytest.raises(ValueError, match="at least 4 real samples, got 3"):
        pr.compute()
    dc.real_features, dc.fake_features = [f, f[:1]], [f]
    with pytest.raises(ValueError, match="at least 6 real samples, got 5"):
        dc.compute()
    dc.real_features, dc.fake_features = [f, f], []
    with pytest.raises(ValueError, match="no fake samples"):
        dc.compute()
    pr.reset()
    assert pr.real_features == [] and pr.fake_features == []
    for m in (pr, dc):
        with pytest.raises(MvdError, match="GPU only"):
            m.update(torch.zeros(2, 3, 32, 32, dtype=torch.uint8), real=True)
        with pytest.raises(MvdError, match="GPU only"):
            m.update_features(torch.zeros(2, 2048), real=False)
    with pytest.raises(MvdError, match="GPU only"):
        knn_radii(torch.zeros(8, 64), 3)
    with pytest.raises(MvdError, match="GPU only"):
        manifold_counts(torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(8, dtype=torch.float64), True)


def test_tower_sharing_with_a_stub_tower():
    """one tower object serves both metrics (and FID / KID): the classes keep the object they are given and build none of their own;
    an image batch on the CPU is refused BEFORE the tower is called"""
    from mvd_amd.fid import FrechetInceptionDistance, InceptionV3FeaturesHIP
    from mvd_amd.kid import KernelInceptionDistance
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall

    class StubTower(InceptionV3FeaturesHIP):
        def __init__(self):      # no weights, no library: only the identity of the object matters here
            self.calls = 0

        def __call__(self, imgs):
            self.calls += 1
            raise AssertionError("the tower must not run on the CPU")

    tower = StubTower()
    metrics = (PrecisionRecall(inception=tower, device="cpu"), DensityCoverage(inception=tower, device="cpu"),
               KernelInceptionDistance(inception=tower, device="cpu"), FrechetInceptionDistance(inception=tower, device="cpu"))
    assert all(m.inception is tower for m in metrics)
    for m in metrics[:2]:
        with pytest.raises(MvdError, match="GPU only"):
            m.update(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), real=True)
    assert tower.calls == 0
    for cls in (PrecisionRecall, DensityCoverage):
        with pytest.raises(ValueError, match="InceptionV3FeaturesHIP"):
            cls(inception=object(), device="cpu")


def test_symbols_and_host_checks():
    """the three entry points are exported, and every argument error is reported on the host (no GPU is needed to get one)"""
    lib = L.lib()
    for name in ("mvd_op_knn_radii_workspace_bytes", "mvd_op_knn_radii", "mvd_op_manifold_counts"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    ws_bytes = lib.mvd_op_knn_radii_workspace_bytes
    # parts x n x (k + 1) doubles, rounded up to 256 bytes; never more parts than 64-column tiles; automatic: ceil(2048 / tiles), but
    # at least two tiles a part
    for n, k, force, parts in ((130, 3, 1, 1), (130, 3, 2, 2), (130, 3, 3, 3), (130, 3, 9, 3), (130, 3, 0, 1), (257, 5, 3, 3), (257, 15, 0, 2),
                               (4, 3, 0, 1), (2000, 5, 0, 16), (10000, 3, 0, 14)):
        assert ws_bytes(n, k, force) == -(-parts * n * (k + 1) * 8 // 256) * 256, (n, k, force)
    for n, k, force in ((130, 0, 0), (130, 16, 0), (3, 3, 0), (130, 3, -1), (130, 3, 65536)):
        assert ws_bytes(n, k, force) < 0 and "n >= k + 1" in L.last_error()
    p = C.c_void_p(4096)      # aligned, never dereferenced: every call below fails its host checks
    knn = lambda **a: lib.mvd_op_knn_radii(a.get("f", p), a.get("n", 130), a.get("d", 64), a.get("k", 3), a.get("parts", 0), a.get("out", p), None, p,      # noqa: E731
                                           a.get("ws", 1 << 20), None)
    assert knn(k=0) == -1 and "1 <= k <= 15" in L.last_error()
    assert knn(k=16) == -1 and knn(n=3) == -1 and knn(parts=-1) == -1
    assert knn(d=96) == -1 and "multiple of 64" in L.last_error()
    assert knn(d=0) == -1
    assert knn(f=C.c_void_p(4100)) == -1 and "misaligned" in L.last_error()
    assert knn(ws=8) == -4 and "workspace" in L.last_error()
    assert knn(f=None) == -1 and knn(out=None) == -1 and "null" in L.last_error()
    cnt = lambda **a: lib.mvd_op_manifold_counts(a.get("q", p), a.get("nq", 8), p, a.get("nr", 8), a.get("d", 64), a.get("rad", p), a.get("closed", 1),      # noqa: E731
                                                 a.get("hq", p), p, None)
    assert cnt(nq=0) == -1 and "nq >= 1" in L.last_error()
    assert cnt(nr=0) == -1
    assert cnt(d=32) == -1 and "multiple of 64" in L.last_error()
    assert cnt(closed=2) == -1 and "closed" in L.last_error()
    assert cnt(q=C.c_void_p(4104)) == -1 and "misaligned" in L.last_error()
    assert cnt(hq=C.c_void_p(4098)) == -1 and "misaligned" in L.last_error()
    assert cnt(q=None) == -1 and cnt(rad=None) == -1 and "null" in L.last_error()
    assert cnt(nq=65536 * 64) == -1 and "too many" in L.last_error()


# ------------------------------------------------------------------------------------------------ fault sensitivity
@pytest.mark.parametrize("n,d", [(130, 64), (257, 2048)])
def test_emulation_of_the_tiling_equals_the_integer_path(n, d):
    """the tiled walk without a fault IS the definition, for every number of parts and both comparisons"""
    dist = P.ternary_d2(n, d, 0)
    dist_qr = P.ternary_d2(150, d, 1, 141, 2)
    for k in (1, 3, 5, 15):
        want_r, want_l = P.radii(None, k, dist).double(), P.knn_list(None, k, dist).double()
        for parts in (1, 2, 3, 5):
            got_r, got_l = P.tiled_knn(dist, k, parts)
            assert torch.equal(got_r, want_r) and torch.equal(got_l, want_l)
    rad = P.radii(None, 3, P.ternary_d2(141, d, 2))
    for closed in (False, True):
        hq, hr = P.tiled_counts(dist_qr, rad, closed)
        want_q, want_r = P.counts(dist_qr, rad, closed)
        assert torch.equal(hq, want_q) and torch.equal(hr, want_r)


@pytest.mark.parametrize("n,d", [(130, 64), (257, 2048)])
def test_each_fault_changes_the_integer_result(n, d):
    """the exact GPU tests compare with ``torch.equal`` on these inputs: each of the faults a tiled implementation can have moves at
    least one of the compared outputs"""
    dist, k = P.ternary_d2(n, d, 0), 3
    want_r, want_l = P.tiled_knn(dist, k, 3)
    knn_faults = ("kth_for_kplus1", "drop_tile_boundary", "drop_part_boundary", "admit_padding")
    assert set(knn_faults) | {"open_for_closed"} == set(P.FAULTS)
    for fault in knn_faults:
        got_r, got_l = P.tiled_knn(dist, k, 3, fault)
        changed = int((got_r != want_r).sum())
        print(f"n {n} d {d} knn {fault}: {changed} radii differ")
        assert changed > 0, fault
    dist_qr = P.ternary_d2(150, d, 1, 141, 2)
    rad = P.radii(None, k, P.ternary_d2(141, d, 2))
    want_q, want_ref = P.tiled_counts(dist_qr, rad, True)
    for fault in ("open_for_closed", "admit_padding"):
        got_q, got_ref = P.tiled_counts(dist_qr, rad, True, fault)
        print(f"n {n} d {d} counts {fault}: {int((got_q != want_q).sum())} query counts, {int((got_ref != want_ref).sum())} reference counts differ")
        assert not torch.equal(got_q, want_q), fault
        assert not torch.equal(got_ref, want_ref), fault
