#!/usr/bin/env python3
"""The guided step under adaptive projected guidance (row N19) at 64x64 and 96x96 latents (rows of 16384 and 36864 floats):
microseconds per launch of

* ``apg``: ``ops.sampler_step_apg`` -- momentum update, five statistics, projection, norm cap and step in ONE launch (the feature);
* ``apg_rescale``: the same launch with guidance rescale 0.7 folded in;
* ``rescaled``: ``ops.sampler_step_rescaled`` of the same build -- the sibling kernel: the same traffic less the momentum buffer's
  read and write;
* ``plain``: ``ops.sampler_step(guidance_scale=...)`` of the same build -- the plain guided step, no statistic: the floor;
* ``eager``: APG as eager torch ops (difference, momentum update, norm and cap, normalise, dot, two broadcasts in double as
  diffusers' ``normalized_guidance`` does them, the combine) followed by ``ops.sampler_step`` of the result -- what a caller
  without the feature would write, and what the feature replaces;

for rows 1, 8, 32, second-order form (history read and written in place, no noise).  The arms alternate in one process and one
window: a sample is ``--inner`` back-to-back calls of one arm between two HIP events, divided by ``--inner``; median and min - max of
``--iters`` samples.  Back-to-back calls measure the larger of the host's launch cost and the device time, which is what a
denoising loop's step pays.  One JSON line to <out-dir>/apg_bench.json.

Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COEFFS = (-0.6, 0.8, 0.5, 0.7, -0.2, 0.0)       # a0, a1, p, q, r, sigma


def eager_step(ops, both, x, hist, mom, gs, eta, tau, beta):
    """output space, in the manner of diffusers' ``normalized_guidance`` (use_original_formulation=True) with its MomentumBuffer"""
    import torch
    u, c = both.chunk(2)
    dims = list(range(1, c.dim()))
    diff = c - u
    mom.mul_(beta).add_(diff)                                               # MomentumBuffer.update
    diff = mom
    if tau > 0.0:
        norm = diff.norm(p=2, dim=dims, keepdim=True)
        diff = diff * torch.minimum(torch.ones_like(norm), tau / norm)
    v0, v1 = diff.double(), torch.nn.functional.normalize(c.double(), dim=dims)
    par = (v0 * v1).sum(dim=dims, keepdim=True) * v1
    orth = v0 - par
    m = c + (gs - 1.0) * (orth.float() + eta * par.float())
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
    ap.add_argument("--rows", default="1,8,32")
    ap.add_argument("--latents", default="64,96", help="latent sides, comma separated: a row is 4 * side * side floats")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--guidance-scale", type=float, default=7.5)
    ap.add_argument("--apg", default="0,15,-0.5", help="eta,norm_threshold,momentum of the APG arms")
    ap.add_argument("--guidance-rescale", type=float, default=0.7, help="of the apg_rescale and rescaled arms")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_apg: needs a GPU (a CPU run measures nothing)")
    from mvd_amd import ops
    from mvd_amd.scheduler import APG
    os.makedirs(a.out_dir, exist_ok=True)
    gs, phi, apg = a.guidance_scale, a.guidance_rescale, APG.of(a.apg)
    a0, a1, p, q, r, sigma = COEFFS
    rec = {"what": "guided DPM-Solver++-form step (history in place, no noise) per call, back-to-back calls between HIP events; arms "
                   "alternate in one window", "guidance_scale": gs, "apg": repr(apg), "guidance_rescale": phi, "iters": a.iters,
           "inner": a.inner, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": [],
           "not_measured": ["device time of the kernel alone (these are back-to-back calls through the host's launch path)",
                            "space='x0'", "rows longer than 36864 floats (the streamed path)", "more than 32 rows",
                            "a full denoising loop with and without APG"]}
    g = torch.Generator().manual_seed(0)
    for side in (int(v) for v in a.latents.split(",")):
        n_row = 4 * side * side
        for rows in (int(v) for v in a.rows.split(",")):
            shape = (rows, 4, side, side)
            both = torch.randn((2 * rows,) + shape[1:], generator=g).cuda()
            x, hist = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
            mom = torch.zeros(shape, device="cuda")
            kw = dict(x0_prev=hist, x0_out=hist)
            arms = {
                "apg": lambda: ops.sampler_step_apg(both, x, gs, a0, a1, p, q, r, sigma, **apg.kwargs(), momentum_buffer=mom, **kw),
                "apg_rescale": lambda: ops.sampler_step_apg(both, x, gs, a0, a1, p, q, r, sigma, **apg.kwargs(), guidance_rescale=phi,
                                                            momentum_buffer=mom, **kw),
                "rescaled": lambda: ops.sampler_step_rescaled(both, x, gs, phi, a0, a1, p, q, r, sigma, **kw),
                "plain": lambda: ops.sampler_step(both, x, a0, a1, p, q, r, sigma, guidance_scale=gs, **kw),
                "eager": lambda: eager_step(ops, both, x, hist, mom, gs, apg.eta, apg.norm_threshold, apg.momentum),
            }
            # the two ways to the APG step agree before they are timed (each from the same history and a zero momentum buffer)
            h0 = hist.clone()
            want = eager_step(ops, both, x, hist, mom, gs, apg.eta, apg.norm_threshold, apg.momentum)
            hist.copy_(h0)
            mom.zero_()
            got = arms["apg"]()
            hist.copy_(h0)
            diff = float((got - want).abs().max() / want.abs().max())
            for _ in range(a.warmup):
                for fn in arms.values():
                    sample_us(fn, a.inner)
            ts = {k: [] for k in arms}
            for _ in range(a.iters):
                for k, fn in arms.items():
                    mom.zero_()                                             # (a geometric series in the buffer stays bounded anyway)
                    ts[k].append(sample_us(fn, a.inner))
            med = {k: statistics.median(v) for k, v in ts.items()}
            spread = max(max(v) - min(v) for v in ts.values())
            bytes_apg = 4 * rows * n_row * (2 + 2 + 2 + 2)                  # u, c, sample, history, M read; out, history, M written
            case = {"rows": rows, "latent": side, "n_row": n_row, "plan": ops.apg_plan(n_row), **{k: stats(v) for k, v in ts.items()},
                    "max_rel_difference_apg_to_eager": diff, "apg_over_rescaled": round(med["apg"] / med["rescaled"], 3),
                    "apg_over_plain": round(med["apg"] / med["plain"], 3), "eager_over_apg": round(med["eager"] / med["apg"], 3),
                    "apg_below_eager": bool(med["apg"] < med["eager"]),
                    "difference_apg_rescaled_beyond_spread": bool(abs(med["apg"] - med["rescaled"]) > spread),
                    "apg_gbytes_per_s_at_median": round(bytes_apg / med["apg"] / 1e3, 1)}
            rec["cases"].append(case)
            print(json.dumps(case), flush=True)
    line = json.dumps(rec)
    with open(os.path.join(a.out_dir, "apg_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
