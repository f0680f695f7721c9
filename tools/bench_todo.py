#!/usr/bin/env python3
"""Token downsampling of the self-attention keys (``MultiViewUNet.enable_todo``): what it costs and what
it saves, beside token merging (N21).  Measurement only.

Full-size SD-2.1 topology (synthetic weights, bench.py's; 64 x 64 latents, camera + image conditioning, the reference cached).  Arms:
off; ToDo (2, 1) nearest; ToDo (2, 1) area; ToDo (2, 2) nearest; token merging at ratio 0.5 (max_downsample 1).
  forward    the batch-1 forward and the 8-view forward under guidance (16 rows);
  operator   at the level-0 blocks' shape (64 x 64, C = 320, fused rows of stride 4C), batch 1 and 16: the self-attention launch at
             nk = 4096 and at nk = 1024 (the pooled K | V buffer, ldk = 2C), and the pooling launch for both methods, as
             microseconds per back-to-back call;
  loop       the 20-step DDIM loop of the 8-view case for every arm, alone and with DeepCache at cache_interval 3.
Off is the baseline, never the code under test.

The protocol is tools/bench_deepcache.py's: same process and window, the arms alternated sample by sample, warm, HIP events around
each sample, each preceded by one untimed call of its arm, median of ``--iters`` with min-max.

NOT measured here: image quality (there are no trained weights), 768 x 768 images, the objects and ragged batch layouts, factors 3
and 4.

Writes one JSON line to <out-dir>/todo_bench.json.  Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import event_ms, stats      # noqa: E402

# arm -> what it sets; "off" first
ARMS = {"off": None, "todo_2_1_nearest": ("todo", 2, 1, "nearest"), "todo_2_1_area": ("todo", 2, 1, "area"),
        "todo_2_2_nearest": ("todo", 2, 2, "nearest"), "tome_0.5": ("tome", 0.5, 1)}


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
        sys.exit("bench_todo: needs a GPU (a CPU run measures nothing)")
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
    rec = {"what": f"arms {list(ARMS)}: one forward (reference cached), the self-attention launch at {hw * hw} and {hw * hw // 4} keys and the "
                   f"pooling launch at {hw}x{hw} x 320, and {a.steps}-step DDIM loops alone and with DeepCache interval 3; SD-2.1 topology, "
                   f"synthetic weights, {hw}x{hw} latents, camera + image conditioning; same process, arms alternated, warm, HIP events, "
                   f"median with min-max",
           "not_measured": "image quality (no trained weights), 768x768 images, the objects and ragged batch layouts, factors 3 and 4",
           "iters": a.iters, "loop_iters": a.loop_iters, "warmup": a.warmup, "steps": a.steps, "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "forward": [], "operator": [], "loop": []}

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def setting(arm):
        what = ARMS[arm]
        model.disable_tome()
        model.disable_todo()
        if what is not None and what[0] == "todo":
            model.enable_todo(*what[1:])
        elif what is not None:
            model.enable_tome(*what[1:])

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
            setting("off")
            base = fwd().clone()
            ms, diff = {r: [] for r in ARMS}, {}
            for i in range(a.warmup + a.iters):
                for r in ARMS:
                    setting(r)
                    out = fwd()                             # untimed: the setting reaches the engine (and the reference is cached)
                    if i == 0:
                        diff[r] = float((out - base).norm() / base.norm())
                    torch.cuda.synchronize()
                    m = event_ms(fwd)
                    if i >= a.warmup:
                        ms[r].append(m)
            med = {r: statistics.median(v) for r, v in ms.items()}
            row = {"forward": name, "rows": int(c["x"].shape[0]), **{r: stats(v) for r, v in ms.items()},
                   **{f"{r}_over_off_median": round(med[r] / med["off"], 4) for r in ARMS if r != "off"},
                   **{f"{r}_rel_l2_vs_off": round(diff[r], 4) for r in ARMS if r != "off"}}
            rec["forward"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        setting("off")

        # ---- the launches at the level-0 blocks' shape, back to back
        C_, heads, N, reps = 320, 5, hw * hw, 20
        for B in (1, 2 * V):
            qkv = torch.randn(B, N, 4 * C_, generator=g).bfloat16().to(dev)
            q, k, v = qkv[:, :, :C_], qkv[:, :, C_:2 * C_], qkv[:, :, 2 * C_:3 * C_]

            def per_call_us(f):
                for _ in range(3):
                    f()
                torch.cuda.synchronize()

                def many():
                    for _ in range(reps):
                        f()
                return [1e3 * event_ms(many) / reps for _ in range(a.iters)]
            kv = ops.todo_downsample(k, v, hw, hw, 2, "nearest")
            op = {"batch": B, "tokens": N, "channels": C_, "keys_pooled": int(kv.shape[1]),
                  "attention_full_us": us_stats(per_call_us(lambda: ops.attention(q, k, v, heads))),
                  "attention_pooled_us": us_stats(per_call_us(lambda: ops.attention(q, kv[:, :, :C_], kv[:, :, C_:], heads))),
                  "pool_nearest_us": us_stats(per_call_us(lambda: ops.todo_downsample(k, v, hw, hw, 2, "nearest", out=kv))),
                  "pool_area_us": us_stats(per_call_us(lambda: ops.todo_downsample(k, v, hw, hw, 2, "area", out=kv)))}
            rec["operator"].append(op)
            print(json.dumps(op), file=sys.stderr, flush=True)

        # ---- the loop: every arm alone, and with DeepCache at interval 3
        name = f"views{V}_guided"
        c = cases[name]
        sched = _make_scheduler(None, "ddim")
        den = MVDDenoiser(model, sched)
        prompt, neg = c["text"][-1:], c["text"][:1]
        lat0 = rnd(c["rows"], 4, hw, hw)
        lkw = dict(num_inference_steps=a.steps, guidance_scale=c["guidance"], negative_prompt_embeds=neg, source_camera=c["src"],
                   target_camera=c["tgt"], source_image_latents=lat1, **c["layout"])
        arms = [(r, iv) for iv in (1, 3) for r in ARMS]

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
               **{f"{r}_interval_{iv}": stats(ms[(r, iv)]) for r, iv in arms},
               **{f"{r}_interval_{iv}_over_off_interval_1_median": round(med[(r, iv)] / med[("off", 1)], 4) for r, iv in arms if (r, iv) != ("off", 1)}}
        rec["loop"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        model.disable_deepcache()
        setting("off")
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "todo_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
