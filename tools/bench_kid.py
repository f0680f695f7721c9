#!/usr/bin/env python3
"""KID and the Inception score on the GPU (row N11): ``KernelInceptionDistance.compute()`` of ``mvd_amd.kid`` at torchmetrics'
defaults (100 subsets of 1000 from 2000 + 2000 features) and at 10 subsets of 100, and ``InceptionScore.compute()`` at n = 2000
(10 splits), on random non-negative features / N(0, 3^2) logits -- no tower runs here.  Warm, HIP events around each call, median
of the repetitions with min / max.  One JSON line to <out-dir>/kid_compute.json.

* ``compute``: the whole call -- the host's ``randperm`` draws, one int32 upload, ``mvd_op_kid_mmd`` (two launches), mean / std;
* ``kernel``: ``mvd_op_kid_mmd`` alone on indices already on the device;
* ``eager_fp64``: the same arithmetic as eager fp64 torch ops on the same device, on the same device-resident indices -- per
  subset a gather, three ``matmul``s, the power, the sums -- alternating with ``kernel`` in one timed window;
* the Inception score likewise: ``compute`` (``randperm``, upload, three launches), and an eager fp64 ``softmax`` /
  ``log_softmax`` / ``chunk`` restatement alternating with it.

Nothing here assumes which side is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_perceptual import stats, timed, timed_alternating      # noqa: E402


def eager_kid(f_real, f_fake, idx, degree, gamma, coef):
    import torch
    x_all, y_all = f_real.double(), f_fake.double()
    m = idx.shape[2]
    vals = []
    for s in range(idx.shape[0]):
        x, y = x_all[idx[s, 0].long()], y_all[idx[s, 1].long()]
        k_xx, k_yy, k_xy = (x @ x.T * gamma + coef) ** degree, (y @ y.T * gamma + coef) ** degree, (x @ y.T * gamma + coef) ** degree
        v = ((k_xx.sum() - k_xx.diag().sum()) + (k_yy.sum() - k_yy.diag().sum())) / (m * (m - 1)) - 2 * k_xy.sum() / m ** 2
        vals.append(v)
    return torch.stack(vals)


def eager_is(logits, perm, splits):
    import torch
    f = logits.double()[perm.long()]
    prob, log_prob = f.softmax(dim=1).chunk(splits, dim=0), f.log_softmax(dim=1).chunk(splits, dim=0)
    return torch.stack([(p * (lp - p.mean(dim=0, keepdim=True).log())).sum(dim=1).mean().exp() for p, lp in zip(prob, log_prob)])


def compare(ta, tb):
    ma, mb = statistics.median(ta), statistics.median(tb)
    return {"eager_over_kernel_median": round(mb / ma, 3), "faster": "kernel" if ma < mb else "eager",
            "difference_beyond_spread": bool(abs(ma - mb) > max(max(ta) - min(ta), max(tb) - min(tb)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100x1000,10x100", help="subsets x subset_size, comma separated")
    ap.add_argument("--features", type=int, default=2000, help="real and fake features each; rows of logits")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_kid: needs a GPU (a CPU run measures nothing)")
    from mvd_amd import ops
    from mvd_amd.fid import InceptionV3FeaturesHIP
    from mvd_amd.kid import InceptionScore, KernelInceptionDistance, kid_subsets
    import fid_ref
    os.makedirs(a.out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(1)
    n, d = a.features, 2048
    f_real = ((0.3 + 0.3 * torch.randn(n, d, generator=g)).abs()).cuda()
    f_fake = ((0.35 + 0.3 * torch.randn(n, d, generator=g)).abs()).cuda()
    rec = {"what": f"KID compute() on {n} + {n} random pool3-like features, Inception-score compute() on {n} x 1008 N(0, 3^2) logits; warm, HIP events",
           "iters": a.iters, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kid": [], }
    tower = InceptionV3FeaturesHIP(fid_ref.synthetic_inception_state_dict(0))      # compute() never runs it: the metrics want one
    for case in a.cases.split(","):
        subsets, m = (int(v) for v in case.split("x"))
        metric = KernelInceptionDistance(subsets=subsets, subset_size=m, inception=tower)
        metric.update_features(f_real, real=True)
        metric.update_features(f_fake, real=False)
        torch.manual_seed(0)
        idx = kid_subsets(n, n, subsets, m).cuda()
        got, want = ops.kid_mmd(f_real, f_fake, idx), eager_kid(f_real, f_fake, idx, 3, 1.0 / d, 1.0)
        tk, te = timed_alternating(lambda: ops.kid_mmd(f_real, f_fake, idx), lambda: eager_kid(f_real, f_fake, idx, 3, 1.0 / d, 1.0), a.warmup, a.iters)
        rec["kid"].append({"subsets": subsets, "subset_size": m, "compute": stats(timed(metric.compute, a.warmup, a.iters)),
                           "kernel": stats(tk), "eager_fp64": dict(stats(te), what="per subset: gather, three fp64 matmuls, power, sums; "
                                                                                   "alternating with kernel"),
                           "max_abs_difference_to_eager": float((got - want).abs().max()), "mean": float(got.mean()),
                           "workspace_bytes": int(ops.L.lib().mvd_op_kid_workspace_bytes(subsets, m)),
                           "fp64_multiply_adds": 3 * subsets * m * m * d, **compare(tk, te)})
    logits = (3.0 * torch.randn(n, 1008, generator=g)).cuda()
    perm = torch.randperm(n, generator=g).to(torch.int32).cuda()
    got, want = ops.inception_score_chunks(logits, perm, 10), eager_is(logits, perm, 10)
    tk, te = timed_alternating(lambda: ops.inception_score_chunks(logits, perm, 10), lambda: eager_is(logits, perm, 10), a.warmup, a.iters)
    score = InceptionScore(splits=10, inception=tower)
    score.features = [logits]
    rec["inception_score"] = {"n": n, "splits": 10, "compute": stats(timed(score.compute, a.warmup, a.iters)), "kernel": stats(tk),
                              "eager_fp64": dict(stats(te), what="fp64 softmax / log_softmax / chunk / mean / sum; alternating with kernel"),
                              "max_rel_difference_to_eager": float(((got - want).abs() / want.abs()).max()), **compare(tk, te)}
    wf = torch.randn(1008, d, generator=g).cuda() * 0.06
    t_fc, t_mm = timed_alternating(lambda: ops.fc_logits(f_real, wf), lambda: f_real @ wf.T, a.warmup, a.iters)
    rec["fc_logits"] = {"n": n, "kernel": stats(t_fc), "eager_fp32_matmul": stats(t_mm), **compare(t_fc, t_mm)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "kid_compute.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
