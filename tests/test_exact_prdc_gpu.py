"""Bit-exact tests of ``mvd_op_knn_radii`` and ``mvd_op_manifold_counts`` (csrc/prdc.hip).

Features uniform over {-1, 0, 1}: every norm, dot product and D2 is an integer below 2^13 and exact in fp64 in any order, so the
expectation is the int64 path of tests/prdc_ref.py and every comparison is ``torch.equal`` -- on ``radii_sq``, on the sorted
(k + 1)-list, on ``hits_per_query`` and on ``hits_per_ref``.  These inputs are full of ties (entries ON the threshold, equal values
inside a list), and tests/test_prdc_cpu.py shows that ``<`` for ``<=``, the k-th value for the (k + 1)-th, a candidate column
dropped at a tile or part boundary and a padded column admitted each change the result on them.  Every feature matrix is a slice
of a larger buffer whose surrounding rows are NaN: a row read outside the matrix would poison the result.  Without csrc/prdc.hip
this file fails at the binding's symbol check."""
import pytest
import torch

import prdc_ref as P

pytestmark = pytest.mark.gpu

GUARD = 4096
PAD_ROWS = 70      # NaN rows before and after: more than a tile


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def guarded(f):
    """the rows of f on the device, inside a buffer whose other rows are NaN"""
    n, d = f.shape
    buf = torch.full((n + 2 * PAD_ROWS, d), float("nan"), dtype=torch.float32, device="cuda")
    buf[PAD_ROWS:PAD_ROWS + n] = f.cuda()
    view = buf[PAD_ROWS:PAD_ROWS + n]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def check_knn(ops, f, dist, k, parts_list):
    """every output of knn_radii on the rows f (host tensor) against the integer distances ``dist``"""
    n = f.shape[0]
    want_list = P.knn_list(None, k, dist).double()
    want = want_list[:, k].contiguous()
    assert torch.equal(want, P.radii(None, k, dist).double())
    fd = guarded(f)
    first = None
    for parts in parts_list:
        need = ops.L.lib().mvd_op_knn_radii_workspace_bytes(n, k, parts)
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        radii, lst = ops.knn_radii(fd, k, force_parts=parts, want_list=True, ws=ws)
        assert radii.dtype == torch.float64 and radii.shape == (n,) and lst.shape == (n, k + 1)
        bad = (radii.cpu() != want).nonzero().flatten().tolist()
        assert torch.equal(radii.cpu(), want), f"radii_sq, parts {parts}: rows {bad[:8]} differ: {radii.cpu()[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
        assert torch.equal(lst.cpu(), want_list), f"sorted list, parts {parts}"
        assert bool((ws[need:] == 0xA5).all()), "wrote beyond the reported workspace size"
        again = ops.knn_radii(fd, k, force_parts=parts)      # knn_sq = NULL, a workspace of its own
        assert torch.equal(again, radii)
        if first is None:
            first = (radii, lst)
        assert torch.equal(first[0], radii) and torch.equal(first[1], lst)      # the bits do not depend on the number of parts


@pytest.mark.parametrize("k", [1, 3, 5, 15])
@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("n", ["k+1", "k+2", 63, 64, 65, 130, 257])
def test_knn_radii_integer_features(ops, n, d, k):
    n = {"k+1": k + 1, "k+2": k + 2}.get(n, n)
    check_knn(ops, P.ternary_features(n, d, 0), P.ternary_d2(n, d, 0), k, (0, 1, 2, 3) if n in (130, 257) else (0,))


@pytest.mark.parametrize("probe", [1, 64, 100, 200])
def test_knn_radii_planted_neighbours(ops, probe):
    """the six nearest neighbours of the probed row sit at columns 0, 63, 64, 127, 128 and n - 1 -- the first and last column of a
    tile, of a part and of the matrix -- each a copy of the row with one coordinate changed; with k = 6 every one of them is in the
    row's list, so a column lost at any of those places changes it"""
    n, d, k = 257, 64, 6
    columns = [c for c in (0, 63, 64, 127, 128, n - 1) if c != probe]
    f = P.planted_features(n, d, 3, (probe,), columns)
    dist = P.d2_int(f, f)
    near = dist[probe].sort().values[:len(columns) + 2]
    assert int(near[0]) == 0 and int(near[len(columns)]) <= 4 and int(near[len(columns) + 1]) > 4      # the planting worked
    assert sorted(dist[probe].argsort(stable=True)[:len(columns) + 1].tolist()) == sorted(columns + [probe])
    check_knn(ops, f, dist, k if len(columns) == 6 else 5, (0, 1, 2, 3, 5))


def check_counts(ops, q, r, dist_qr, radii_r):
    qd, rd, rad = guarded(q), guarded(r), radii_r.double().cuda()
    for closed in (True, False):
        want_q, want_r = P.counts(dist_qr, radii_r, closed)
        hq, hr = ops.manifold_counts(qd, rd, rad, closed)
        assert hq.dtype == torch.int32 and hr.dtype == torch.int32 and hq.shape == (q.shape[0],) and hr.shape == (r.shape[0],)
        assert torch.equal(hq.cpu(), want_q), f"hits_per_query, closed {closed}: {int(hq.sum())} hits, {int(want_q.sum())} expected"
        assert torch.equal(hr.cpu(), want_r), f"hits_per_ref, closed {closed}"
        # the outputs are zeroed by the call, and either may be NULL
        gq = torch.full((q.shape[0] + 64,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        gr = torch.full((r.shape[0] + 64,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        ops.L.call("mvd_op_manifold_counts", ops._p(qd), q.shape[0], ops._p(rd), r.shape[0], q.shape[1], ops._p(rad), int(closed), ops._p(gq), ops._p(gr), ops._s())
        assert torch.equal(gq[:q.shape[0]], hq) and torch.equal(gr[:r.shape[0]], hr)
        assert bool((gq[q.shape[0]:] == 0x7F7F7F7F).all()) and bool((gr[r.shape[0]:] == 0x7F7F7F7F).all()), "wrote beyond an output"
        only_q, none = ops.manifold_counts(qd, rd, rad, closed, want_ref=False)
        assert none is None and torch.equal(only_q, hq)
        none, only_r = ops.manifold_counts(qd, rd, rad, closed, want_query=False)
        assert none is None and torch.equal(only_r, hr)


@pytest.mark.parametrize("k", [1, 3, 5, 15])
@pytest.mark.parametrize("d", [64, 2048])
def test_manifold_counts_two_sets(ops, d, k):
    """nq = 150 queries against nr = 141 references (neither a multiple of the tile), radii of the reference set at k"""
    q, r = P.ternary_features(150, d, 1), P.ternary_features(141, d, 2)
    check_counts(ops, q, r, P.ternary_d2(150, d, 1, 141, 2), P.radii(None, k, P.ternary_d2(141, d, 2)))


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("n", ["k+1", "k+2", 63, 64, 65, 130, 257])
def test_manifold_counts_a_set_with_itself(ops, n, d):
    """every size at which the tiling changes, queries = references: the diagonal (D2 = 0) and every tie of the set's own radii"""
    k = 3
    n = {"k+1": k + 1, "k+2": k + 2}.get(n, n)
    f, dist = P.ternary_features(n, d, 0), P.ternary_d2(n, d, 0)
    check_counts(ops, f, f, dist, P.radii(None, k, dist))


def test_rejects_bad_arguments(ops):
    from mvd_amd._lib import MvdError
    f = P.ternary_features(63, 64, 0).cuda()
    with pytest.raises(MvdError, match="n >= k \\+ 1"):
        ops.knn_radii(f[:3].contiguous(), 3)
    with pytest.raises(MvdError, match="1 <= k <= 15"):
        ops.knn_radii(f, 16)
    with pytest.raises(MvdError, match="multiple of 64"):
        ops.knn_radii(f[:, :32].contiguous(), 3)
    with pytest.raises(MvdError, match="multiple of 64"):
        ops.manifold_counts(f[:, :32].contiguous(), f[:, :32].contiguous(), torch.zeros(63, dtype=torch.float64, device="cuda"), True)
