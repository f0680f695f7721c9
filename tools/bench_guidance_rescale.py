#!/usr/bin/env python3
"""The guided step with guidance rescale (row N17) at the latent sizes of 512^2 and 768^2 images: microseconds per call of

* ``fused``: ``ops.sampler_step_rescaled`` -- statistics, combine, rescale and step in ONE launch (the feature);
* ``plain``: today's ``ops.sampler_step(guidance_scale=...)`` -- the same step without the rescale: the floor, it reads and writes
  the same tensors and computes no statistic;
* ``eager``: the rescale as eager torch ops (chunk, combine, two ``std`` over the row, the blend) followed by ``ops.sampler_step``
  of the result -- what a caller without the feature would write, and what the feature replaces;

for rows 1, 8, 32, 64 x n_row 16384 and 36864, second-order form (history read and written in place, no noise).  The three arms
alternate in one process: a sample is ``--inner`` back-to-back calls of one arm between two HIP events, divided by ``--inner``;
median and min - max of ``--iters`` samples.  Back-to-back calls measure the larger of the host's launch cost and the device
time, which is what a denoising loop's step pays.  One JSON line to <out-dir>/guidance_rescale_bench.json.

Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COEFFS = (-0.6, 0.8, 0.5, 0.7, -0.2, 0.0)       # a0, a1, p, q, r, sigma


def eager_step(ops, both, x, hist, gs, phi):
    u, c = both.chunk(2)
    m = u + gs * (c - u)
    dims = list(range(1, c.dim()))
    m = phi * (m * (c.std(dim=dims, keepdim=True) / m.std(dim=dims, keepdim=True))) + (1.0 - phi) * m
    a0, a1, p, q, r, sigma = COEFFS
    return ops.sampler_step(m, x, a0, a1, p, q, r, sigma, x0_prev=hist, x0_out=hist)


def sample_us(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def stats(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,32,64")
    ap.add_argument("--n-rows", default="16384,36864", help="floats per row, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--guidance-scale", type=float, default=7.5)
    ap.add_argument("--guidance-rescale", type=float, default=0.7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_guidance_rescale: needs a GPU (a CPU run measures nothing)")
    from mvd_amd import ops
    os.makedirs(a.out_dir, exist_ok=True)
    gs, phi = a.guidance_scale, a.guidance_rescale
    a0, a1, p, q, r, sigma = COEFFS
    rec = {"what": "guided DPM-Solver++-form step (history in place, no noise) per call, back-to-back calls between HIP events; arms alternate",
           "guidance_scale": gs, "guidance_rescale": phi, "iters": a.iters, "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "cases": []}
    g = torch.Generator().manual_seed(0)
    for n_row in (int(v) for v in a.n_rows.split(",")):
        for rows in (int(v) for v in a.rows.split(",")):
            shape = (rows, 4, n_row // 4)
            both = torch.randn((2 * rows,) + shape[1:], generator=g).cuda()
            x, hist = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
            arms = {
                "fused": lambda: ops.sampler_step_rescaled(both, x, gs, phi, a0, a1, p, q, r, sigma, x0_prev=hist, x0_out=hist),
                "plain": lambda: ops.sampler_step(both, x, a0, a1, p, q, r, sigma, x0_prev=hist, x0_out=hist, guidance_scale=gs),
                "eager": lambda: eager_step(ops, both, x, hist, gs, phi),
            }
            # the two ways to the rescaled step agree before they are timed (each from the same history)
            h0 = hist.clone()
            want = eager_step(ops, both, x, hist, gs, phi)
            hist.copy_(h0)
            got = arms["fused"]()
            hist.copy_(h0)
            diff = float((got - want).abs().max() / want.abs().max())
            for _ in range(a.warmup):
                for fn in arms.values():
                    sample_us(fn, a.inner)
            ts = {k: [] for k in arms}
            for _ in range(a.iters):
                for k, fn in arms.items():
                    ts[k].append(sample_us(fn, a.inner))
            med = {k: statistics.median(v) for k, v in ts.items()}
            spread = max(max(v) - min(v) for v in ts.values())
            bytes_fused = 4 * rows * n_row * (2 + 2 + 2)            # u, c, sample, history read; sample-sized out, history written
            case = {"rows": rows, "n_row": n_row, "plan": ops.cfg_rescale_plan(n_row), **{k: stats(v) for k, v in ts.items()},
                    "max_rel_difference_fused_to_eager": diff, "fused_over_plain": round(med["fused"] / med["plain"], 3),
                    "eager_over_fused": round(med["eager"] / med["fused"], 3), "fused_below_eager": bool(med["fused"] < med["eager"]),
                    "difference_fused_eager_beyond_spread": bool(abs(med["fused"] - med["eager"]) > spread),
                    "fused_gbytes_per_s_at_median": round(bytes_fused / med["fused"] / 1e3, 1)}
            rec["cases"].append(case)
            print(json.dumps(case), flush=True)
    line = json.dumps(rec)
    with open(os.path.join(a.out_dir, "guidance_rescale_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
