#!/usr/bin/env python3
"""DeepCache (``MultiViewUNet.enable_deepcache``): what a shallow step saves.  Measurement only.

Full-size SD-2.1 topology (synthetic weights, bench.py's; 64 x 64 latents, camera + image conditioning), two forwards:
  batch1     one sample row with the full conditioning (infer.py's forward), no guidance;
  views8     the 8-view shared-reference forward under guidance: 8 views x 2 rows = 16 rows (``views=8``).
For each:
  forward    ms per FULL forward with the reference cached (``cache_reference``: a step of a loop after the first) against ms per
             SHALLOW forward of branch 0 and of branch 1 -- three arms, alternated sample by sample;
  loop       ms per 20-step DDIM loop (``MVDDenoiser``; the whole loop, scheduler steps included, first step cold) at
             cache_interval 1, 2, 3 and 5 (branch 0) -- four arms, alternated sample by sample.  Interval 1 is the loop without
             DeepCache.

The protocol is tools/bench_freeu.py's: same process and window, the arms alternated sample by sample, warm, HIP events around
each sample, each sample preceded by one untimed call of its arm (for a shallow forward: the refresh forward that stores the
feature, then one shallow forward), median of ``--iters`` with min-max.

Writes one JSON line to <out-dir>/deepcache_bench.json.  Nothing here assumes which arm is faster, and nothing is said about
image quality (there are no trained weights).  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import event_ms, stats      # noqa: E402

INTERVALS = (1, 2, 3, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64: 512 x 512 images)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_deepcache: needs a GPU (a CPU run measures nothing)")
    from bench import fill_synthetic_weights
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    from mvd_amd.pipeline import MVDDenoiser, _make_scheduler
    from mvd_amd.utils import orbit_cameras
    os.makedirs(a.out_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    model = MultiViewUNet(None, unet_config=UNetConfig.sd21(), init="empty", img_ref_scale=0.3, cam_modulation_strength=0.2,
                          dedup_encoder_weights=False).to(dev)
    model.eval()
    fill_synthetic_weights(model, 0)
    g = torch.Generator().manual_seed(3)
    hw, V = a.latent, a.views
    enc_dim = 6 * ((model.cam_output_dim // 2) // 3)
    model.fourier_projection = (torch.randn(model.cam_output_dim, enc_dim, generator=g) / enc_dim ** 0.5).to(dev)
    model.cache_reference = True
    t = torch.tensor(500)
    rec = {"what": f"DeepCache: full forward (reference cached) vs shallow forward of branch 0 / 1, and {a.steps}-step DDIM loops at cache_interval "
                   f"{INTERVALS}; SD-2.1 topology, synthetic weights, {hw}x{hw} latents, camera + image conditioning; same process, arms "
                   f"alternated, warm, HIP events, median of {a.iters} with min-max",
           "iters": a.iters, "warmup": a.warmup, "steps": a.steps, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "forward": [], "loop": []}

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    lat1 = 0.18215 * rnd(1, 4, hw, hw)
    cases = {
        "batch1": dict(x=rnd(1, 4, hw, hw), text=rnd(1, 77, 1024), layout={}, guidance=1.0, rows=1,
                       src=orbit_cameras(1).to(dev), tgt=orbit_cameras(1, start_deg=40.0).to(dev)),
        f"views{V}_guided": dict(x=rnd(2 * V, 4, hw, hw), text=rnd(2, 77, 1024), layout=dict(views=V), guidance=7.5, rows=V,
                                 src=orbit_cameras(1).expand(V, -1, -1).contiguous().to(dev),
                                 tgt=orbit_cameras(V, elevation_deg=15.0, start_deg=20.0).to(dev)),
    }
    with torch.no_grad():
        for name, c in cases.items():
            kw = dict(source_camera=c["src"], target_camera=c["tgt"], source_image_latents=lat1, **c["layout"])

            def fwd(deep=None):
                return model(c["x"], t, c["text"], **kw, **({"deep_cache": deep} if deep else {})).sample

            # ---- one forward: full (reference cached) | shallow branch 0 | shallow branch 1
            def arm(which):
                if which == "full":
                    model.disable_deepcache()
                    fwd()                                   # untimed: the setting reaches the engine (and the reference is cached)
                    return lambda: fwd()
                model.enable_deepcache(2, int(which[-1]))
                fwd("refresh")                              # untimed: stores the feature (a new branch drops the old one)
                fwd("reuse")
                return lambda: fwd("reuse")

            model.reset_reference_cache()
            arms = ("full", "shallow_b0", "shallow_b1")
            ms = {k: [] for k in arms}
            for i in range(a.warmup + a.iters):
                for k in arms:
                    f = arm(k)
                    torch.cuda.synchronize()
                    m = event_ms(f)
                    if i >= a.warmup:
                        ms[k].append(m)
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {"forward": name, "rows": int(c["x"].shape[0]), **{k: stats(v) for k, v in ms.items()},
                   "shallow_b0_over_full_median": round(med["shallow_b0"] / med["full"], 4),
                   "shallow_b1_over_full_median": round(med["shallow_b1"] / med["full"], 4)}
            rec["forward"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)

            # ---- the loop
            sched = _make_scheduler(None, "ddim")
            den = MVDDenoiser(model, sched)
            prompt, neg = c["text"][-1:], (c["text"][:1] if c["guidance"] > 1.0 else None)
            lat0 = rnd(c["rows"], 4, hw, hw)
            lkw = dict(num_inference_steps=a.steps, guidance_scale=c["guidance"], negative_prompt_embeds=neg, source_camera=c["src"],
                       target_camera=c["tgt"], source_image_latents=lat1, **c["layout"])

            def loop(interval):
                if interval == 1:
                    model.disable_deepcache()
                else:
                    model.enable_deepcache(interval, 0)
                return den(prompt, latents=lat0.clone(), **lkw)

            ms = {n: [] for n in INTERVALS}
            for i in range(a.warmup + a.iters):
                for n in INTERVALS:
                    loop(n)                                 # untimed
                    torch.cuda.synchronize()
                    m = event_ms(lambda: loop(n))
                    if i >= a.warmup:
                        ms[n].append(m)
            med = {n: statistics.median(v) for n, v in ms.items()}
            row = {"loop": name, "rows": int(c["x"].shape[0]), "steps": a.steps, **{f"interval_{n}": stats(v) for n, v in ms.items()},
                   **{f"interval_{n}_over_interval_1_median": round(med[n] / med[1], 4) for n in INTERVALS if n != 1}}
            rec["loop"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            model.disable_deepcache()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "deepcache_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
