#!/usr/bin/env python3
"""Token merging (``MultiViewUNet.enable_tome``): what it costs and what it saves.  Measurement only.

Full-size SD-2.1 topology (synthetic weights, bench.py's; 64 x 64 latents, camera + image conditioning, the reference cached), token
merging off against on at ratio 0.25, 0.5 and 0.75 (max_downsample 1: the five full-resolution blocks):
  forward    the batch-1 forward and the 8-view forward under guidance (16 rows);
  operator   at the merging blocks' shape (64 x 64, C = 320), batch 1 and 16: match + select (two launches), merge, un-merge + add,
             and the self-attention launch at 4096 keys against N' = 4096 - r, as microseconds per back-to-back call;
  loop       the 20-step DDIM loop of the 8-view case with token merging alone and with DeepCache at cache_interval 3.
Off is the baseline, never the code under test.

The protocol is tools/bench_deepcache.py's: same process and window, the arms alternated sample by sample, warm, HIP events around
each sample, each preceded by one untimed call of its arm, median of ``--iters`` with min-max.

NOT measured here: image quality (there are no trained weights), 768 x 768 images, the objects and ragged batch layouts.

Writes one JSON line to <out-dir>/tome_bench.json.  Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import event_ms, stats      # noqa: E402

RATIOS = (0.0, 0.25, 0.5, 0.75)


def us_stats(us):
    """median / min / max of microsecond samples, under keys that say so"""
    return {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64: 512 x 512 images)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tome: needs a GPU (a CPU run measures nothing)")
    from bench import fill_synthetic_weights
    from mvd_amd import ops
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
    rec = {"what": f"token merging off vs ratio {RATIOS[1:]} (max_downsample 1): one forward (reference cached), the operators at {hw}x{hw} x 320, "
                   f"and {a.steps}-step DDIM loops alone and with DeepCache interval 3; SD-2.1 topology, synthetic weights, {hw}x{hw} latents, "
                   f"camera + image conditioning; same process, arms alternated, warm, HIP events, median with min-max",
           "not_measured": "image quality (no trained weights), 768x768 images, the objects and ragged batch layouts",
           "iters": a.iters, "loop_iters": a.loop_iters, "warmup": a.warmup, "steps": a.steps, "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "forward": [], "operator": [], "loop": []}

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def setting(ratio):
        if ratio > 0.0:
            model.enable_tome(ratio, 1)
        else:
            model.disable_tome()

    lat1 = 0.18215 * rnd(1, 4, hw, hw)
    cases = {
        "batch1": dict(x=rnd(1, 4, hw, hw), text=rnd(1, 77, 1024), layout={}, guidance=1.0, rows=1,
                       src=orbit_cameras(1).to(dev), tgt=orbit_cameras(1, start_deg=40.0).to(dev)),
        f"views{V}_guided": dict(x=rnd(2 * V, 4, hw, hw), text=rnd(2, 77, 1024), layout=dict(views=V), guidance=7.5, rows=V,
                                 src=orbit_cameras(1).expand(V, -1, -1).contiguous().to(dev),
                                 tgt=orbit_cameras(V, elevation_deg=15.0, start_deg=20.0).to(dev)),
    }
    with torch.no_grad():
        # ---- one forward
        for name, c in cases.items():
            kw = dict(source_camera=c["src"], target_camera=c["tgt"], source_image_latents=lat1, **c["layout"])

            def fwd():
                return model(c["x"], t, c["text"], **kw).sample
            model.reset_reference_cache()
            setting(0.0)
            base = fwd().clone()
            ms, diff = {r: [] for r in RATIOS}, {}
            for i in range(a.warmup + a.iters):
                for r in RATIOS:
                    setting(r)
                    out = fwd()                             # untimed: the setting reaches the engine (and the reference is cached)
                    if i == 0:
                        diff[r] = float((out - base).norm() / base.norm())
                    torch.cuda.synchronize()
                    m = event_ms(fwd)
                    if i >= a.warmup:
                        ms[r].append(m)
            med = {r: statistics.median(v) for r, v in ms.items()}
            row = {"forward": name, "rows": int(c["x"].shape[0]), **{f"ratio_{r}": stats(v) for r, v in ms.items()},
                   **{f"ratio_{r}_over_off_median": round(med[r] / med[0.0], 4) for r in RATIOS[1:]},
                   **{f"ratio_{r}_rel_l2_vs_off": round(diff[r], 4) for r in RATIOS[1:]}}
            rec["forward"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        setting(0.0)

        # ---- the operators at the merging blocks' shape, back to back
        C_, heads, N, reps = 320, 5, hw * hw, 20
        for B in (1, 2 * V):
            x = torch.randn(B, N, C_, generator=g).bfloat16().to(dev)
            h = torch.randn(B, N, C_, generator=g).bfloat16().to(dev)
            qkv = torch.randn(B, N, 3 * C_, generator=g).bfloat16().to(dev)

            def per_call_us(f):
                for _ in range(3):
                    f()
                torch.cuda.synchronize()

                def many():
                    for _ in range(reps):
                        f()
                return [1e3 * event_ms(many) / reps for _ in range(a.iters)]
            full_q = qkv
            op = {"batch": B, "tokens": N, "channels": C_,
                  "attention_full_us": us_stats(per_call_us(lambda: ops.attention(full_q[:, :, :C_], full_q[:, :, C_:2 * C_], full_q[:, :, 2 * C_:], heads)))}
            for ratio in RATIOS[1:]:
                r = int(N * ratio)
                slot, members, starts = ops.tome_match(x, hw, hw, r)
                merged = ops.tome_merge(x, hw, hw, r, members, starts)
                mq = torch.randn(B, N - r, 3 * C_, generator=g).bfloat16().to(dev)
                op[f"ratio_{ratio}"] = {
                    "rows": N - r,
                    "match_select_us": us_stats(per_call_us(lambda: ops.tome_match(x, hw, hw, r))),
                    "merge_us": us_stats(per_call_us(lambda: ops.tome_merge(x, hw, hw, r, members, starts, out=merged))),
                    "unmerge_add_us": us_stats(per_call_us(lambda: ops.tome_unmerge_add(h, merged, hw, hw, r, slot))),
                    "attention_us": us_stats(per_call_us(lambda: ops.attention(mq[:, :, :C_], mq[:, :, C_:2 * C_], mq[:, :, 2 * C_:], heads)))}
            rec["operator"].append(op)
            print(json.dumps(op), file=sys.stderr, flush=True)

        # ---- the loop: token merging alone, and with DeepCache at interval 3
        name = f"views{V}_guided"
        c = cases[name]
        sched = _make_scheduler(None, "ddim")
        den = MVDDenoiser(model, sched)
        prompt, neg = c["text"][-1:], c["text"][:1]
        lat0 = rnd(c["rows"], 4, hw, hw)
        lkw = dict(num_inference_steps=a.steps, guidance_scale=c["guidance"], negative_prompt_embeds=neg, source_camera=c["src"],
                   target_camera=c["tgt"], source_image_latents=lat1, **c["layout"])
        arms = [(r, iv) for iv in (1, 3) for r in RATIOS]

        def loop(arm):
            setting(arm[0])
            if arm[1] == 1:
                model.disable_deepcache()
            else:
                model.enable_deepcache(arm[1], 0)
            return den(prompt, latents=lat0.clone(), **lkw)
        ms = {arm: [] for arm in arms}
        for i in range(a.warmup + a.loop_iters):
            for arm in arms:
                if i == 0:
                    loop(arm)                               # untimed, once: workspace, reference, first-use initialisation
                torch.cuda.synchronize()
                m = event_ms(lambda: loop(arm))
                if i >= a.warmup:
                    ms[arm].append(m)
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        row = {"loop": name, "rows": int(c["x"].shape[0]), "steps": a.steps,
               **{f"ratio_{r}_interval_{iv}": stats(ms[(r, iv)]) for r, iv in arms},
               **{f"ratio_{r}_interval_{iv}_over_off_interval_1_median": round(med[(r, iv)] / med[(0.0, 1)], 4) for r, iv in arms if (r, iv) != (0.0, 1)}}
        rec["loop"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        model.disable_deepcache()
        setting(0.0)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "tome_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
