#!/usr/bin/env python3
"""The UniPC step (row N23) at 64x64 and 96x96 latents (rows of 16384 and 36864 floats): microseconds per call of

* ``unipc``: ``ops.unipc_step`` -- the guidance combine, the x0 conversion, the corrector of the previous step and the predictor
  of this one in ONE launch (the feature), with the coefficients ``UniPCMultistepScheduler`` gives in mid-schedule (order 2, bh2,
  corrector on): reads u, c, the sample, the last sample and two x0 predictions, writes the next sample, the corrected sample
  (over the last sample) and the new x0 (over the oldest prediction);
* ``eager``: the same update as a chain of eager torch ops, written the way diffusers' ``UniPCMultistepScheduler.step`` writes it
  (combine, ``convert_model_output``, D1 differences, the corrector, the history shift, the predictor) -- what a caller without
  the feature would run;
* ``dpm2m``: ``ops.sampler_step(guidance_scale=...)`` with DPM-Solver++ 2M coefficients of the same step, history in place -- the
  yardstick of what a step of the loop costs today;

for rows 1, 8, 32.  The arms alternate in one process and one window: a sample is ``--inner`` back-to-back calls of one arm
between two HIP events, divided by ``--inner``; median and min - max of ``--iters`` samples.  Back-to-back calls measure the larger
of the host's launch cost and the device time, which is what a denoising loop's step pays.  One JSON line to
<out-dir>/unipc_bench.json.

Nothing here assumes which arm is faster, and no target time is set.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def eager_step(both, gs, x, state, e):
    """diffusers' step on torch tensors: ``state`` = [last_sample, m_prev (older x0), m0 (newer x0)]; returns the next sample and
    replaces the state.  ``e``: the step's scalars (dict) in the textbook form."""
    u, c = both.chunk(2)
    m = u + gs * (c - u)
    x0 = e["alpha_s"] * x - e["sbar_s"] * m                                  # v_prediction
    last, m1, m0 = state
    # UniC, order 2, from the previous sigma to this one
    d1 = (m1 - m0) / e["c_rk"]
    xc = e["c_ratio"] * last - e["c_alpha_t"] * e["c_phi1"] * m0
    xc = xc - e["c_alpha_t"] * e["c_B"] * (e["c_rho0"] * d1 + e["c_rho1"] * (x0 - m0))
    # UniP, order 2, from this sigma to the next
    d1 = (m0 - x0) / e["p_rk"]
    y = e["p_ratio"] * xc - e["p_alpha_t"] * e["p_phi1"] * x0
    y = y - e["p_alpha_t"] * e["p_B"] * (0.5 * d1)
    state[0], state[1], state[2] = xc, m0, x0
    return y


def textbook_scalars(s, i):
    """the scalars of ``eager_step`` for call ``i`` of scheduler ``s`` (order 2, bh2), from its sigmas"""
    import math
    import numpy as np

    def asl(k):
        sg = s._sig[k]
        alpha = 1.0 / math.sqrt(sg * sg + 1.0)
        return alpha, sg * alpha, math.log(alpha) - math.log(sg * alpha)

    e = {}
    e["alpha_s"], e["sbar_s"], _ = asl(i)
    for tag, s0 in (("c", i - 1), ("p", i)):
        alpha_t, sbar_t, lam_t = asl(s0 + 1)
        _, sbar_s0, lam_s0 = asl(s0)
        h = lam_t - lam_s0
        rk = (asl(s0 - 1)[2] - lam_s0) / h
        phi1 = math.expm1(-h)
        e.update({f"{tag}_ratio": sbar_t / sbar_s0, f"{tag}_alpha_t": alpha_t, f"{tag}_phi1": phi1, f"{tag}_B": phi1, f"{tag}_rk": rk})
        if tag == "c":
            hh = -h
            b0 = (phi1 / hh - 1.0) / phi1
            b1 = ((phi1 / hh - 1.0) / hh - 0.5) * 2.0 / phi1
            rho = np.linalg.solve(np.array([[1.0, 1.0], [rk, 1.0]]), np.array([b0, b1]))
            e["c_rho0"], e["c_rho1"] = float(rho[0]), float(rho[1])
    return e


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
    ap.add_argument("--steps", type=int, default=10, help="the schedule the coefficients are taken from")
    ap.add_argument("--step-index", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_unipc: needs a GPU (a CPU run measures nothing)")
    from mvd_amd import ops
    from mvd_amd.pipeline import _make_scheduler
    os.makedirs(a.out_dir, exist_ok=True)
    gs, i = a.guidance_scale, a.step_index
    uni, dpm = _make_scheduler(None, "unipc"), _make_scheduler(None, "dpmsolver++")
    uni.set_timesteps(a.steps)
    dpm.set_timesteps(a.steps)
    c = uni.step_coefficients(i)
    assert c.corr and c.p1 != 0.0 and c.c1 != 0.0 and c.p2 == 0.0, "pick a step in mid-schedule (order 2, corrector on)"
    e = textbook_scalars(uni, i)
    d = dpm.step_coefficients(i)
    rec = {"what": "one guided step of the denoising loop per call, back-to-back calls between HIP events; arms alternate in one window",
           "guidance_scale": gs, "schedule_steps": a.steps, "step_index": i, "unipc_coefficients": c._asdict(), "iters": a.iters,
           "inner": a.inner, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": [],
           "not_measured": ["device time of the kernel alone (these are back-to-back calls through the host's launch path)",
                            "order 3", "the two-launch path with guidance rescale or APG", "more than 32 rows",
                            "a full denoising loop with UniPC against DPM-Solver++ at its step count", "image quality"]}
    g = torch.Generator().manual_seed(0)
    for side in (int(v) for v in a.latents.split(",")):
        n_row = 4 * side * side
        for rows in (int(v) for v in a.rows.split(",")):
            shape = (rows, 4, side, side)
            both = torch.randn((2 * rows,) + shape[1:], generator=g).cuda()
            x, last, h0, h1 = (torch.randn(shape, generator=g).cuda() for _ in range(4))
            hist = h0.clone()
            state = [last.clone(), h1.clone(), h0.clone()]
            arms = {
                "unipc": lambda: ops.unipc_step(both, x, c.a0, c.a1, c.px, c.p0, c.p1, c.p2, corr=True, cx=c.cx, c0=c.c0, c1=c.c1,
                                                c2=c.c2, ct=c.ct, last_sample=last, h0=h0, h1=h1, guidance_scale=gs, xc_out=last,
                                                x0_out=h1),
                "eager": lambda: eager_step(both, gs, x, state, e),
                "dpm2m": lambda: ops.sampler_step(both, x, *d[:5], guidance_scale=gs, x0_prev=hist, x0_out=hist),
            }
            # the two ways to the UniPC step agree before they are timed (each from the same state)
            want = eager_step(both, gs, x, [last.clone(), h1.clone(), h0.clone()], e)
            keep = (last.clone(), h1.clone())
            got = arms["unipc"]()
            last.copy_(keep[0])
            h1.copy_(keep[1])
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
            bytes_unipc = 4 * rows * n_row * (6 + 3)                        # u, c, sample, last, h0, h1 read; y, xc, x0 written
            case = {"rows": rows, "latent": side, "n_row": n_row, **{k: stats(v) for k, v in ts.items()},
                    "max_rel_difference_unipc_to_eager": diff, "eager_over_unipc": round(med["eager"] / med["unipc"], 3),
                    "unipc_over_dpm2m": round(med["unipc"] / med["dpm2m"], 3), "unipc_below_eager": bool(med["unipc"] < med["eager"]),
                    "difference_unipc_dpm2m_beyond_spread": bool(abs(med["unipc"] - med["dpm2m"]) > spread),
                    "unipc_gbytes_per_s_at_median": round(bytes_unipc / med["unipc"] / 1e3, 1)}
            rec["cases"].append(case)
            print(json.dumps(case), flush=True)
    line = json.dumps(rec)
    with open(os.path.join(a.out_dir, "unipc_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
