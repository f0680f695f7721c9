"""Improved precision / recall (torch-fidelity's ``prc``) and density / coverage (the ``prdc`` package) restated in fp64 torch --
neither package is installed where this project runs, so this file is what the kernels of csrc/prdc.hip are compared with;
tests/test_prdc_cpu.py checks it against the packages where they import.

* ``d2`` / ``radii`` / ``knn_list`` / ``predicate`` / ``precision_recall`` / ``density_coverage``: the formulas of
  mvd_amd/prdc.py's docstring on fp64 copies of the features, all on SQUARED distances in Gram form.
* ``d2_int`` and the ``*_int`` functions: the exact integer path, int64 ``((a[:, None] - b[None]) ** 2).sum(-1)``, ``kthvalue``,
  counts.  On ``ternary_features`` every D2 is an integer below 2^13, so the GPU comparison is ``torch.equal``.
* ``tiled_knn`` / ``tiled_counts``: a CPU emulation of the kernels' tiling (64-column tiles, column parts, a (k + 1)-list per row
  and part, a merge; masked tile sums), with switchable faults -- tests/test_prdc_cpu.py shows that each fault changes the result
  on the integer inputs, i.e. that the exact GPU tests would see it.
* ``gram_bound`` / ``min_margin``: the rounding bound of a Gram-form D2 and the smallest distance of a predicate entry from its
  threshold in units of it.

Plain helper module (like kid_ref.py), no fixtures."""
import functools

import torch

TILE = 64


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def d2(a, b):
    """(na, nb) fp64: max(0, |a|^2 + |b|^2 - 2 a.b)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None] - 2.0 * (a @ b.T)).clamp_(min=0.0)


def knn_list(f, k, dist=None):
    """(n, k + 1): every row's k + 1 smallest D2 to the rows of f, itself included, ascending"""
    dist = d2(f, f) if dist is None else dist
    return dist.sort(dim=1).values[:, :k + 1].contiguous()


def radii(f, k, dist=None):
    """(n,): kthvalue(k + 1) of every row of D2(f, f)"""
    dist = d2(f, f) if dist is None else dist
    return dist.kthvalue(k + 1, dim=1).values


def predicate(dist_qr, radii_r, closed):
    """P[j][i] = D2(q_j, r_i) <= radii_r[i] (closed) or < (open)"""
    return dist_qr <= radii_r[None] if closed else dist_qr < radii_r[None]


def counts(dist_qr, radii_r, closed):
    """(hits_per_query, hits_per_ref) int32"""
    p = predicate(dist_qr, radii_r, closed)
    return p.sum(1).to(torch.int32), p.sum(0).to(torch.int32)


def _pr_from(d_fr, r_real, r_fake, strict):
    precision = int(predicate(d_fr, r_real, not strict).any(1).sum()) / d_fr.shape[0]
    recall = int(predicate(d_fr.T, r_fake, not strict).any(1).sum()) / d_fr.shape[1]
    return precision, recall, 2 * precision * recall / max(precision + recall, 1e-5)


def precision_recall(real, fake, k=3, strict=False):
    """(precision, recall, f_score) as Python floats"""
    return _pr_from(d2(fake, real), radii(real, k), radii(fake, k), strict)


def _dc_from(d_fr, r_real, k):
    p = predicate(d_fr, r_real, False)
    return int(p.sum()) / (k * d_fr.shape[0]), int(p.any(0).sum()) / d_fr.shape[1]


def density_coverage(real, fake, k=5):
    """(density, coverage) as Python floats"""
    return _dc_from(d2(fake, real), radii(real, k), k)


# ------------------------------------------------------------------------------------------------ the exact integer path
def d2_int(a, b, rows=16):
    """(na, nb) int64 ``((a[:, None] - b[None]) ** 2).sum(-1)``, in row batches to bound the memory"""
    a, b = a.detach().cpu().long(), b.detach().cpu().long()
    return torch.cat([((a[i:i + rows, None] - b[None]) ** 2).sum(-1) for i in range(0, a.shape[0], rows)])


def precision_recall_int(real, fake, k=3, strict=False):
    return _pr_from(d2_int(fake, real), radii(real, k, d2_int(real, real)), radii(fake, k, d2_int(fake, fake)), strict)


def density_coverage_int(real, fake, k=5):
    return _dc_from(d2_int(fake, real), radii(real, k, d2_int(real, real)), k)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=16)
def ternary_features(n, d, seed):
    """(n, d) fp32 uniform over {-1, 0, 1}: every D2 is an integer <= 4 d, full of ties -- shared, do not modify"""
    g = torch.Generator().manual_seed(6000 + seed)
    return torch.randint(-1, 2, (n, d), generator=g).float()


@functools.lru_cache(maxsize=16)
def ternary_d2(n, d, seed, m=None, seed2=None):
    """int64 D2 of ternary_features(n, d, seed) against itself, or against ternary_features(m, d, seed2) -- shared, do not modify"""
    a = ternary_features(n, d, seed)
    return d2_int(a, a if m is None else ternary_features(m, d, seed2))


@functools.lru_cache(maxsize=16)
def lowrank_features(n, seed, scale=1.0, shift=0.0, d=2048, rank=8):
    """non-negative low-rank rows |z A| scale + shift, z (n, rank), A (rank, d): precision / recall / density / coverage of two such
    sets are well inside (0, 1) at a few hundred rows, where plain Gaussian rows at d = 2048 give a degenerate precision near 0;
    A depends on d and rank alone, z on the seed -- shared, do not modify"""
    ga = torch.Generator().manual_seed(7000)
    a = torch.randn(rank, d, generator=ga)
    g = torch.Generator().manual_seed(7001 + seed)
    return ((torch.randn(n, rank, generator=g) @ a).abs() * scale + shift).contiguous()


def planted_features(n, d, seed, probes, columns):
    """ternary rows where, for every probed row p, the rows at ``columns`` are copies of row p with ONE coordinate changed (D2 = 1
    or 4 from p; everything else is near 4 d / 3 ... ): the nearest neighbours of p sit exactly at those columns"""
    f = ternary_features(n, d, seed).clone()
    g = torch.Generator().manual_seed(6500 + seed)
    for p in probes:
        for c in columns:
            if c == p:
                continue
            f[c] = f[p]
            j = int(torch.randint(0, d, (1,), generator=g))
            f[c, j] = 1.0 if f[c, j] != 1.0 else 0.0
    return f


# ------------------------------------------------------------------------------------------------ rounding bound and margins
def gram_bound(q, r, d=None):
    """(nq, nr): 4 d 2^-53 (|q|^2 + |r|^2) -- a dot product and two norms of d terms each carry gamma_d = d 2^-53 relative to
    |q|^2 + |r|^2 >= 2 |q.r| ... in all 2 d 2^-53 (|q|^2 + |r|^2), with a factor 2 of slack"""
    q, r = q.detach().cpu().double(), r.detach().cpu().double()
    d = q.shape[1] if d is None else d
    return 4.0 * d * 2.0 ** -53 * ((q * q).sum(1)[:, None] + (r * r).sum(1)[None])


def min_margin(q, r, radii_r):
    """min over the predicate's entries of |D2 - radius| / gram_bound: above 2, neither side's rounding can flip an entry (the
    radius is itself a D2 of the reference set, so it carries at most a bound of its own)"""
    return float(((d2(q, r) - radii_r[None]).abs() / gram_bound(q, r)).min())


# ------------------------------------------------------------------------------------------------ CPU emulation of the tiling
FAULTS = ("open_for_closed", "kth_for_kplus1", "drop_tile_boundary", "drop_part_boundary", "admit_padding")


def _parts(tiles, parts):
    parts = min(parts, tiles)
    return [(p * tiles // parts, (p + 1) * tiles // parts) for p in range(parts)]


def tiled_knn(dist, k, parts=1, fault=None):
    """``dist`` (n, n): the kernel's walk -- per column part a (k + 1)-list per row, fed tile by tile with the columns < n, then the
    k + 1 smallest of the parts' lists -> (radii (n,), lists (n, k + 1)).  A padded column stands for the clamped row n - 1."""
    n = dist.shape[0]
    tiles = -(-n // TILE)
    inf = torch.full((n, k + 1), float("inf"), dtype=torch.float64)
    part_lists = []
    for pi, (t0, t1) in enumerate(_parts(tiles, parts)):
        lst = inf.clone()
        for t in range(t0, t1):
            cols = list(range(t * TILE, min((t + 1) * TILE, n)))
            if fault == "admit_padding" and (t + 1) * TILE > n:
                cols.append(n - 1)      # one padded column (the clamped last row) admitted as a candidate
            if fault == "drop_tile_boundary" and t > 0:
                cols = cols[1:]         # the first column of a tile dropped
            if fault == "drop_part_boundary" and t == t0 and pi > 0:
                cols = cols[1:]         # the first column of a part dropped
            lst = torch.cat([lst, dist[:, cols].double()], 1).sort(dim=1).values[:, :k + 1]
        part_lists.append(lst)
    merged = torch.cat(part_lists, 1).sort(dim=1).values[:, :k + 1]
    return (merged[:, k - 1] if fault == "kth_for_kplus1" else merged[:, k]).clone(), merged


def tiled_counts(dist_qr, radii_r, closed, fault=None):
    """tile by tile: predicate, mask rows >= nq and columns >= nr, add the tile's row and column sums -> int32 pair"""
    nq, nr = dist_qr.shape
    if fault == "open_for_closed":
        closed = False
    hq, hr = torch.zeros(nq, dtype=torch.int32), torch.zeros(nr, dtype=torch.int32)
    for r0 in range(0, nq, TILE):
        for c0 in range(0, nr, TILE):
            rows = torch.arange(r0, min(r0 + TILE, nq))
            cols = torch.arange(c0, c0 + TILE)
            live = cols < nr
            if fault == "admit_padding":
                live = live | (cols == nr)      # the first padded column counted: it stands for the clamped row nr - 1
            cc = cols.clamp(max=nr - 1)
            p = predicate(dist_qr[rows][:, cc].double(), radii_r[cc].double(), closed) & live[None]
            hq[rows] += p.sum(1).to(torch.int32)
            hr.index_add_(0, cc, p.sum(0).to(torch.int32))
    return hq, hr
