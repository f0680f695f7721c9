#!/usr/bin/env python3
"""O objects x V views: ONE object forward (``MultiViewUNet.forward(..., views=V, objects=O)``) against
the two things a user could run before it.  Measurement only.

Arms, per (O, V, g):
  objects     one object forward of g O V rows;
  sequential  the O shared-reference forwards (``views=V``, N14), one object after the other -- the same function;
  repeated    ONE ordinary forward of g O V rows with every row's source repeated (``source_image_latents`` of g O V rows).
              This arm computes ANOTHER function (encoder pass at batch g O V, batch-coupled Q2 statistics, Q4 over the wrong
              rows): its time is what the only other single call costs, not an alternative implementation.

Full-size SD-2.1 topology, synthetic weights (bench.py's), 64 x 64 latents, camera + image conditioning, (O, V) in {(2, 4), (4, 4),
(8, 4), (4, 8)}, g in {1, 2}, ``cold`` (the encoder pass runs in every forward) and ``cached`` (``cache_reference``: the forwards
of a denoising loop after the first; the engine holds ONE reference, so the sequential arm's cached sample is the sum over the
objects of one timed forward each, every one primed by an untimed forward of the same object -- a step of O ``generate_views``
loops run one after the other).  The protocol is tools/bench_views.py's: same process and window, arms alternated sample by
sample, warm, HIP events around each arm's whole work, each sample preceded by one untimed call of its arm (workspace binding
and, cached, the arm's reference), median of ``--iters``.

Writes one JSON line to <out-dir>/objects_bench.json.  Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
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
    ap.add_argument("--shapes", default="2x4,4x4,8x4,4x8", help="O x V, comma separated")
    ap.add_argument("--rows-per-view", default="1,2", help="g: 1, or 2 under classifier-free guidance")
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64: 512 x 512 images)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_objects: needs a GPU (a CPU run measures nothing)")
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
    g = torch.Generator().manual_seed(3)
    hw = a.latent
    enc_dim = 6 * ((model.cam_output_dim // 2) // 3)
    model.fourier_projection = (torch.randn(model.cam_output_dim, enc_dim, generator=g) / enc_dim ** 0.5).to(dev)
    t = torch.tensor(500)
    rec = {"what": f"one object forward of O objects x V views against the O sequential shared-reference forwards (the same function) and "
                   f"against ONE ordinary forward with the sources repeated per row (ANOTHER function: batch-coupled statistics, "
                   f"encoder pass at batch g O V); SD-2.1 topology, synthetic weights, {hw}x{hw} latents, camera + image conditioning; "
                   f"same process, alternated, warm, HIP events",
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": []}
    with torch.no_grad():
        for gg in (int(v) for v in a.rows_per_view.split(",")):
            for O, V in (tuple(int(n) for n in s.split("x")) for s in a.shapes.split(",")):
                n = O * V
                x = torch.randn(n, 4, hw, hw, generator=g).to(dev)
                sample = torch.cat([x] * gg)                                          # row j O V + o V + v
                text = torch.randn(gg * O, 77, 1024, generator=g).to(dev)             # row j O + o
                lat = (0.18215 * torch.randn(O, 4, hw, hw, generator=g)).to(dev)
                src = torch.cat([orbit_cameras(1, start_deg=10.0 * o) for o in range(O)]).to(dev).repeat_interleave(V, 0).contiguous()
                tgt = torch.cat([orbit_cameras(V, elevation_deg=15.0, start_deg=20.0 + 7.0 * o) for o in range(O)]).to(dev)
                rows = [[j * n + o * V + v for j in range(gg) for v in range(V)] for o in range(O)]
                per_obj = [dict(x=sample[rows[o]].contiguous(), text=text[[j * O + o for j in range(gg)]].contiguous(),
                                lat=lat[o:o + 1].contiguous(), src=src[o * V:(o + 1) * V].contiguous(),
                                tgt=tgt[o * V:(o + 1) * V].contiguous()) for o in range(O)]
                text_rows = text.repeat_interleave(V, 0).contiguous()
                lat_rows = lat.repeat_interleave(V, 0).repeat(gg, 1, 1, 1).contiguous()
                cam_rows = dict(source_camera=src.repeat(gg, 1, 1).contiguous(), target_camera=tgt.repeat(gg, 1, 1).contiguous())

                def objects():
                    return model(sample, t, text, source_camera=src, target_camera=tgt, source_image_latents=lat, views=V, objects=O).sample

                def shared(p):
                    return model(p["x"], t, p["text"], source_camera=p["src"], target_camera=p["tgt"], source_image_latents=p["lat"],
                                 views=V).sample

                def sequential():
                    return [shared(p) for p in per_obj]

                def sequential_cached_ms():
                    total = 0.0
                    for p in per_obj:
                        shared(p)                                 # untimed: this object's reference into the cache
                        torch.cuda.synchronize()
                        total += event_ms(lambda: shared(p))
                    return total

                def repeated():
                    return model(sample, t, text_rows, source_image_latents=lat_rows, **cam_rows).sample

                arms = (("objects", objects), ("sequential", sequential), ("repeated", repeated))
                # objects and sequential compute the same thing (bf16 noise apart), repeated does not: checked once, untimed
                model.cache_reference = False
                got = objects()
                want = torch.empty_like(got)
                for o, out in enumerate(sequential()):
                    want[rows[o]] = out
                diff = float((got - want).norm() / want.norm())
                diff_rep = float((repeated() - want).norm() / want.norm())
                for mode in ("cold", "cached"):
                    model.cache_reference = mode == "cached"
                    model.reset_reference_cache()
                    ms = {name: [] for name, _ in arms}
                    for i in range(a.warmup + a.iters):
                        for name, fn in arms:
                            fn()                                  # untimed: this arm's workspace binding (and cached reference)
                            torch.cuda.synchronize()
                            m = sequential_cached_ms() if (mode == "cached" and name == "sequential") else event_ms(fn)
                            if i >= a.warmup:
                                ms[name].append(m)
                    med = {name: statistics.median(v) for name, v in ms.items()}
                    spread = max(max(ms[k]) - min(ms[k]) for k in ("objects", "sequential"))
                    case = {"objects": O, "views": V, "rows_per_view": gg, "mode": mode,
                            "object_forward": stats(ms["objects"]), "sequential_shared": stats(ms["sequential"]),
                            "repeated_sources_other_function": stats(ms["repeated"]),
                            "sequential_over_objects_median": round(med["sequential"] / med["objects"], 3),
                            "repeated_over_objects_median": round(med["repeated"] / med["objects"], 3),
                            "ms_per_view_objects": round(med["objects"] / n, 3), "ms_per_view_sequential": round(med["sequential"] / n, 3),
                            "fastest": min(med, key=med.get),
                            "objects_vs_sequential_beyond_spread": bool(abs(med["objects"] - med["sequential"]) > spread),
                            "rel_l2_objects_vs_sequential": round(diff, 5), "rel_l2_repeated_vs_sequential": round(diff_rep, 5)}
                    rec["cases"].append(case)
                    print(json.dumps(case), file=sys.stderr, flush=True)
                model.cache_reference = False
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "objects_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
