#!/usr/bin/env python3
"""Ragged turntables: ONE ragged forward (``MultiViewUNet.forward(..., views=(V_0, ..))``) against the three
things a user could run before it.  Measurement only.

The layouts are the validation run's own: with ``max_views_per_object = 4`` every object gives three sources with 3, 2 and 1
target views, so n validation objects are the view counts (3, 2, 1) x n -- O = 3 n references, R = 6 n views.

Arms, per (n, g):
  ragged      one ragged forward of g R rows;
  sequential  the O shared-reference forwards (``views=V_o``, N14), one source after the other -- the same function;
  padded      the uniform object forward (``views=3, objects=O``, N15) on the layout padded to V = 3: g 9 n rows, one third of them
              wasted -- the same function on the rows that count;
  repeated    ONE ordinary forward of the same g R rows with every view's own source repeated to R rows -- what
              ``mvd_amd/val.py`` calls today.  This arm computes ANOTHER function (encoder pass at batch R, batch-coupled Q2
              statistics, Q4 over the wrong rows): its time is what the only other single call costs.

Full-size SD-2.1 topology, synthetic weights (bench.py's), 64 x 64 latents, camera + image conditioning, n in {1, 2, 4}, g in {1, 2},
``cold`` (the encoder pass runs in every forward) and ``cached`` (``cache_reference``: the forwards of a denoising loop after the
first; the engine holds ONE reference, so the sequential arm's cached sample is the sum over the sources of one timed forward
each, every one primed by an untimed forward of the same source).  The protocol is tools/bench_objects.py's: same process and
window, arms alternated sample by sample, warm, HIP events around each arm's whole work, each sample preceded by one untimed
call of its arm, median of ``--iters`` with min-max.

Writes one JSON line to <out-dir>/ragged_bench.json.  Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
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
    ap.add_argument("--objects", default="1,2,4", help="validation objects n: the layout is (3, 2, 1) x n")
    ap.add_argument("--rows-per-view", default="1,2", help="g: 1, or 2 under classifier-free guidance")
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64: 512 x 512 images)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ragged: needs a GPU (a CPU run measures nothing)")
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
    rec = {"what": f"one ragged forward of view counts (3, 2, 1) x n against the O sequential shared-reference forwards and the uniform "
                   f"object forward padded to V = 3 (the same function) and against ONE ordinary forward with the sources repeated per "
                   f"view (ANOTHER function: batch-coupled statistics, encoder pass at batch R); SD-2.1 topology, synthetic weights, "
                   f"{hw}x{hw} latents, camera + image conditioning; same process, alternated, warm, HIP events",
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": []}
    with torch.no_grad():
        for gg in (int(v) for v in a.rows_per_view.split(",")):
            for n in (int(v) for v in a.objects.split(",")):
                counts = (3, 2, 1) * n
                O, R, V = len(counts), sum(counts), 3
                obj = [o for o, c in enumerate(counts) for _ in range(c)]
                offs = [sum(counts[:o]) for o in range(O)]
                x = torch.randn(R, 4, hw, hw, generator=g).to(dev)
                sample = torch.cat([x] * gg)                                          # row j R + c
                text = torch.randn(gg * O, 77, 1024, generator=g).to(dev)             # row j O + o
                lat = (0.18215 * torch.randn(O, 4, hw, hw, generator=g)).to(dev)
                src_o = torch.cat([orbit_cameras(1, start_deg=10.0 * o) for o in range(O)]).to(dev)
                src = src_o[obj].contiguous()
                tgt = torch.cat([orbit_cameras(counts[o], elevation_deg=15.0, start_deg=20.0 + 7.0 * o) for o in range(O)]).to(dev)
                rows = [[j * R + offs[o] + v for j in range(gg) for v in range(counts[o])] for o in range(O)]
                per_obj = [dict(x=sample[rows[o]].contiguous(), text=text[[j * O + o for j in range(gg)]].contiguous(),
                                lat=lat[o:o + 1].contiguous(), src=src[offs[o]:offs[o] + counts[o]].contiguous(),
                                tgt=tgt[offs[o]:offs[o] + counts[o]].contiguous(), V=counts[o]) for o in range(O)]
                # repeated sources: what val.py's pipeline call hands the UNet -- g R sample rows, text per row, R source rows
                text_rows = torch.cat([text[[j * O + o for o in obj]] for j in range(gg)]).contiguous()
                lat_rows = lat[obj].contiguous()
                cam_rows = dict(source_camera=src.repeat(gg, 1, 1).contiguous(), target_camera=tgt.repeat(gg, 1, 1).contiguous())
                # padded to V = 3: view slot o V + v holds view min(v, V_o - 1) of object o (the surplus rows are wasted work)
                pad = [offs[o] + min(v, counts[o] - 1) for o in range(O) for v in range(V)]
                pad_sample = torch.cat([x[pad]] * gg).contiguous()
                pad_src, pad_tgt = src[pad].contiguous(), tgt[pad].contiguous()
                keep = [j * O * V + o * V + v for j in range(gg) for o in range(O) for v in range(counts[o])]     # -> row j R + c

                def ragged():
                    return model(sample, t, text, source_camera=src, target_camera=tgt, source_image_latents=lat, views=counts).sample

                def shared(p):
                    return model(p["x"], t, p["text"], source_camera=p["src"], target_camera=p["tgt"], source_image_latents=p["lat"],
                                 views=p["V"]).sample

                def sequential():
                    return [shared(p) for p in per_obj]

                def sequential_cached_ms():
                    total = 0.0
                    for p in per_obj:
                        shared(p)                                 # untimed: this source's reference into the cache
                        torch.cuda.synchronize()
                        total += event_ms(lambda: shared(p))
                    return total

                def padded():
                    return model(pad_sample, t, text, source_camera=pad_src, target_camera=pad_tgt, source_image_latents=lat, views=V,
                                 objects=O).sample

                def repeated():
                    return model(sample, t, text_rows, source_image_latents=lat_rows, **cam_rows).sample

                arms = (("ragged", ragged), ("sequential", sequential), ("padded", padded), ("repeated", repeated))
                # ragged, sequential and padded compute the same thing (bf16 noise apart), repeated does not: checked once, untimed
                model.cache_reference = False
                got = ragged()
                want = torch.empty_like(got)
                for o, out in enumerate(sequential()):
                    want[rows[o]] = out
                rel = lambda y: float((y - want).norm() / want.norm())          # noqa: E731
                diff, diff_pad, diff_rep = rel(got), rel(padded()[keep]), rel(repeated())
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
                    case = {"validation_objects": n, "view_counts": list(counts), "sources": O, "views": R, "rows_per_view": gg, "mode": mode,
                            "ragged_forward": stats(ms["ragged"]), "sequential_shared": stats(ms["sequential"]),
                            "padded_object_forward": stats(ms["padded"]), "repeated_sources_other_function": stats(ms["repeated"]),
                            "sequential_over_ragged_median": round(med["sequential"] / med["ragged"], 3),
                            "padded_over_ragged_median": round(med["padded"] / med["ragged"], 3),
                            "repeated_over_ragged_median": round(med["repeated"] / med["ragged"], 3),
                            "ms_per_view_ragged": round(med["ragged"] / R, 3), "fastest": min(med, key=med.get),
                            "rel_l2_ragged_vs_sequential": round(diff, 5), "rel_l2_padded_vs_sequential": round(diff_pad, 5),
                            "rel_l2_repeated_vs_sequential": round(diff_rep, 5)}
                    rec["cases"].append(case)
                    print(json.dumps(case), file=sys.stderr, flush=True)
                model.cache_reference = False
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "ragged_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
