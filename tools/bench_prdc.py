#!/usr/bin/env python3
"""Precision / recall and density / coverage on the GPU (row N12): ``knn_radii``, ``manifold_counts`` and the two ``compute()``
calls of ``mvd_amd.prdc`` at 2000 + 2000 and 10000 + 10000 features, on random non-negative low-rank features -- no tower runs
here.  Warm, HIP events around each call, median of the repetitions with min / max.  One JSON line to
<out-dir>/prdc_compute.json.

* ``kernel``: the operator alone (``mvd_op_knn_radii``: two launches; ``mvd_op_manifold_counts``: two memsets and one launch);
* ``eager_fp64``: the same arithmetic as eager fp64 torch ops on the same device, alternating with ``kernel`` in one timed window:
  the Gram form ``|a|^2 + |b|^2 - 2 a.b`` in row batches (the n x n matrix in fp64 is 800 MB at n = 10000), ``kthvalue(k + 1)``
  per batch for the radii, comparison and row / column sums for the counts.  Nothing else here can stand in as a reference;
* ``compute``: the whole call of ``PrecisionRecall`` (two k-NN passes, two count passes) and ``DensityCoverage`` (one each).

Nothing here assumes which side is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_kid import compare      # noqa: E402
from bench_perceptual import stats, timed, timed_alternating      # noqa: E402

BATCH = 2000      # rows of the eager side's distance block: 2000 x 10000 fp64 = 160 MB


def eager_d2(a, na, b, nb):
    return (na[:, None] + nb[None] - 2.0 * (a @ b.T)).clamp_(min=0.0)


def eager_radii(f, k):
    import torch
    x = f.double()
    nx = (x * x).sum(1)
    return torch.cat([eager_d2(x[i:i + BATCH], nx[i:i + BATCH], x, nx).kthvalue(k + 1, dim=1).values for i in range(0, x.shape[0], BATCH)])


def eager_counts(q, r, radii, closed):
    import torch
    x, y = q.double(), r.double()
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    hq, hr = [], torch.zeros(y.shape[0], dtype=torch.int64, device=q.device)
    for i in range(0, x.shape[0], BATCH):
        dist = eager_d2(x[i:i + BATCH], nx[i:i + BATCH], y, ny)
        p = dist <= radii[None] if closed else dist < radii[None]
        hq.append(p.sum(1))
        hr += p.sum(0)
    return torch.cat(hq).to(torch.int32), hr.to(torch.int32)


def features(n, seed, scale, shift, d=2048, rank=8):
    import torch
    ga = torch.Generator().manual_seed(7000)
    a = torch.randn(rank, d, generator=ga)
    g = torch.Generator().manual_seed(7001 + seed)
    return ((torch.randn(n, rank, generator=g) @ a).abs() * scale + shift).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000", help="real and fake features each, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_prdc: needs a GPU (a CPU run measures nothing)")
    from mvd_amd import ops
    from mvd_amd.fid import InceptionV3FeaturesHIP
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    import fid_ref
    os.makedirs(a.out_dir, exist_ok=True)
    d = 2048
    rec = {"what": "knn_radii, manifold_counts and the compute() calls of PrecisionRecall (k = 3, <=) and DensityCoverage (k = 5, <) on n + n "
                   "non-negative low-rank features of 2048 floats; warm, HIP events", "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "eager_row_batch": BATCH, "cases": []}
    tower = InceptionV3FeaturesHIP(fid_ref.synthetic_inception_state_dict(0))      # compute() never runs it: the metrics want one
    for n in (int(v) for v in a.sizes.split(",")):
        real, fake = features(n, 0, 1.0, 0.0), features(n, 1, 1.1, 0.2)
        case = {"n": n, "fp64_multiply_adds_per_pass": n * n * d}
        for k in (3, 5):
            got, want = ops.knn_radii(real, k), eager_radii(real, k)
            tk, te = timed_alternating(lambda: ops.knn_radii(real, k), lambda: eager_radii(real, k), a.warmup, a.iters)
            case[f"knn_radii_k{k}"] = {"kernel": stats(tk), "eager_fp64": stats(te), "max_rel_difference_to_eager": float(((got - want).abs() / want).max()),
                                       "workspace_bytes": int(ops.L.lib().mvd_op_knn_radii_workspace_bytes(n, k, 0)), **compare(tk, te)}
        for k, closed in ((3, True), (5, False)):
            radii = ops.knn_radii(real, k)
            got, want = ops.manifold_counts(fake, real, radii, closed), eager_counts(fake, real, radii, closed)
            tk, te = timed_alternating(lambda: ops.manifold_counts(fake, real, radii, closed), lambda: eager_counts(fake, real, radii, closed), a.warmup, a.iters)
            case[f"manifold_counts_k{k}_{'closed' if closed else 'open'}"] = {
                "kernel": stats(tk), "eager_fp64": stats(te), "hits": int(got[0].sum()),
                "counts_differing_from_eager": int((got[0] != want[0]).sum()) + int((got[1] != want[1]).sum()), **compare(tk, te)}
        pr, dc = PrecisionRecall(inception=tower), DensityCoverage(inception=tower)
        for m in (pr, dc):
            m.update_features(real, real=True)
            m.update_features(fake, real=False)
        case["precision_recall"] = {"compute": stats(timed(pr.compute, a.warmup, a.iters)), "value": [float(v) for v in pr.compute()]}
        case["density_coverage"] = {"compute": stats(timed(dc.compute, a.warmup, a.iters)), "value": [float(v) for v in dc.compute()]}
        rec["cases"].append(case)
        del real, fake, pr, dc
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "prdc_compute.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
