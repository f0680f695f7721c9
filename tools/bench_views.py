#!/usr/bin/env python3
"""V views of one object: ONE shared-reference forward (``MultiViewUNet.forward(..., views=V)``) against
the V sequential batch-g forwards it replaces (the loop of infer.py:111-122 through the unchanged path).  Measurement only.

Full-size SD-2.1 topology, synthetic weights (bench.py's), 512 x 512 images (64 x 64 latents), camera + image conditioning,
V in {2, 4, 8, 16}, g in {1, 2} (2 = classifier-free guidance: [uncond x V | cond x V]), ``cold`` (the reference encoder pass runs
in every forward) and ``cached`` (``cache_reference``: the forwards of a denoising loop after the first).  Both arms run in the
same process and window, alternated sample by sample, warm, HIP events around each arm's whole work (the V sequential calls
are ONE sample).  The engine holds one reference cache and one bound workspace shape, so each arm's sample is preceded by
one untimed call of that arm: it re-binds the arm's workspace and, in ``cached`` mode, restores the arm's cached reference.

Writes one JSON line to <out-dir>/views_bench.json (the table of DESIGN.md section 9 N14 / BASELINE.md).  Nothing here assumes
which arm is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import event_ms, stats      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="2,4,8,16")
    ap.add_argument("--rows-per-view", default="1,2", help="g: 1, or 2 under classifier-free guidance")
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64: 512 x 512 images)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_views: needs a GPU (a CPU run measures nothing)")
    from bench import fill_synthetic_weights
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    from mvd_amd.utils import orbit_cameras
    os.makedirs(a.out_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    model = MultiViewUNet(None, unet_config=UNetConfig.sd21(), init="empty", img_ref_scale=0.3, cam_modulation_strength=0.2,
                          dedup_encoder_weights=False).to(dev)
    model.eval()
    fill_synthetic_weights(model, 0)
    g = torch.Generator().manual_seed(2)
    hw = a.latent
    enc_dim = 6 * ((model.cam_output_dim // 2) // 3)
    model.fourier_projection = (torch.randn(model.cam_output_dim, enc_dim, generator=g) / enc_dim ** 0.5).to(dev)
    text2 = torch.randn(2, 77, 1024, generator=g).to(dev)
    lat = (0.18215 * torch.randn(1, 4, hw, hw, generator=g)).to(dev)
    t = torch.tensor(500)
    src1 = orbit_cameras(1).to(dev)
    rec = {"what": f"one shared-reference forward of V views against V sequential batch-g forwards; SD-2.1 topology, synthetic weights, "
                   f"{hw}x{hw} latents, camera + image conditioning; same process, alternated, warm, HIP events",
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": []}
    with torch.no_grad():
        for gg in (int(v) for v in a.rows_per_view.split(",")):
            for V in (int(v) for v in a.views.split(",")):
                x = torch.randn(V, 4, hw, hw, generator=g).to(dev)
                sample = torch.cat([x] * gg)
                text = text2[:gg]
                tgt = orbit_cameras(V, elevation_deg=15.0, start_deg=20.0).to(dev)
                src = src1.expand(V, -1, -1).contiguous()
                rows = [[j * V + v for j in range(gg)] for v in range(V)]
                per_view = [sample[r].contiguous() for r in rows]

                def shared():
                    return model(sample, t, text, source_camera=src, target_camera=tgt, source_image_latents=lat, views=V).sample

                def sequential():
                    return [model(per_view[v], t, text, source_camera=src1, target_camera=tgt[v:v + 1], source_image_latents=lat).sample
                            for v in range(V)]

                # the two arms compute the same thing (bf16 noise apart): checked once, outside the timed window
                model.cache_reference = False
                got, want = shared(), torch.cat(sequential())
                order = [r for v in range(V) for r in rows[v]]
                diff = float((got[order] - want).norm() / want.norm())
                for mode in ("cold", "cached"):
                    model.cache_reference = mode == "cached"
                    model.reset_reference_cache()
                    ts, tq = [], []
                    for i in range(a.warmup + a.iters):
                        shared()                              # untimed: this arm's workspace binding (and cached reference)
                        torch.cuda.synchronize()
                        ms_s = event_ms(shared)
                        sequential()
                        torch.cuda.synchronize()
                        ms_q = event_ms(sequential)
                        if i >= a.warmup:
                            ts.append(ms_s)
                            tq.append(ms_q)
                    ms, mq = statistics.median(ts), statistics.median(tq)
                    case = {"views": V, "rows_per_view": gg, "mode": mode, "shared": stats(ts), "sequential": stats(tq),
                            "sequential_over_shared_median": round(mq / ms, 3), "faster": "shared" if ms < mq else "sequential",
                            "difference_beyond_spread": bool(abs(ms - mq) > max(max(ts) - min(ts), max(tq) - min(tq))),
                            "rel_l2_between_arms": round(diff, 5)}
                    rec["cases"].append(case)
                    print(json.dumps(case), file=sys.stderr, flush=True)
                model.cache_reference = False
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "views_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
