#!/usr/bin/env python3
"""FreeU (``MultiViewUNet.enable_freeu``): what the six extra launches of a forward cost.  Measurement only.

Two forwards of the full-size SD-2.1 topology (synthetic weights, bench.py's; 64 x 64 latents, camera + image conditioning), each
with FreeU off and on (the published SD-2.1 setting s1 = 0.9, s2 = 0.2, b1 = 1.4, b2 = 1.6):
  batch1     one sample row with the full conditioning (infer.py's forward);
  objects    the 8 x 4 object forward under guidance: 8 objects x 4 views x 2 rows = 64 rows (``views=4, objects=8``).
``cold``: the encoder pass runs in every forward; ``cached``: ``cache_reference``, the forwards of a denoising loop after the first
(the cached reference does not depend on FreeU, so toggling keeps it).

The protocol is tools/bench_ragged.py's: same process and window, the two arms alternated sample by sample, warm, HIP events around
each forward, each sample preceded by one untimed call of its arm, median of ``--iters`` with min-max.  Also timed: the operator
alone (``ops.freeu``) at the six shapes of a forward, per batch.

Writes one JSON line to <out-dir>/freeu_bench.json.  Nothing here assumes which arm is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import event_ms, stats      # noqa: E402

SETTING = dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64: 512 x 512 images)")
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_freeu: needs a GPU (a CPU run measures nothing)")
    from bench import fill_synthetic_weights
    from mvd_amd import ops
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
    hw, O, V = a.latent, a.objects, a.views
    enc_dim = 6 * ((model.cam_output_dim // 2) // 3)
    model.fourier_projection = (torch.randn(model.cam_output_dim, enc_dim, generator=g) / enc_dim ** 0.5).to(dev)
    t = torch.tensor(500)
    rec = {"what": f"one forward with FreeU off and on ({SETTING}); SD-2.1 topology, synthetic weights, {hw}x{hw} latents, camera + image "
                   f"conditioning; same process, arms alternated, warm, HIP events, median of {a.iters} with min-max",
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": [], "operator": []}

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    one = dict(x=rnd(1, 4, hw, hw), text=rnd(1, 77, 1024), kw=dict(source_camera=orbit_cameras(1).to(dev), target_camera=orbit_cameras(1, start_deg=40.0).to(dev),
                                                                  source_image_latents=0.18215 * rnd(1, 4, hw, hw)))
    rows = 2 * O * V
    many = dict(x=rnd(rows, 4, hw, hw), text=rnd(2 * O, 77, 1024),
                kw=dict(source_camera=torch.cat([orbit_cameras(1, start_deg=10.0 * o) for o in range(O) for _ in range(V)]).to(dev),
                        target_camera=torch.cat([orbit_cameras(V, elevation_deg=15.0, start_deg=20.0 + 7.0 * o) for o in range(O)]).to(dev),
                        source_image_latents=0.18215 * rnd(O, 4, hw, hw), views=V, objects=O))
    with torch.no_grad():
        for name, c in (("batch1", one), (f"objects_{O}x{V}_guided", many)):
            def fwd():
                return model(c["x"], t, c["text"], **c["kw"]).sample

            def arm(on):
                if on:
                    model.enable_freeu(**SETTING)
                else:
                    model.disable_freeu()
                return fwd

            model.cache_reference = False
            off_out = arm(False)().clone()
            on_out = arm(True)().clone()
            diff = float((on_out - off_out).norm() / off_out.norm())
            for mode in ("cold", "cached"):
                model.cache_reference = mode == "cached"
                model.reset_reference_cache()
                ms = {False: [], True: []}
                for i in range(a.warmup + a.iters):
                    for on in (False, True):
                        f = arm(on)
                        f()                               # untimed: the setting reaches the engine, the workspace is bound (and the reference cached)
                        torch.cuda.synchronize()
                        m = event_ms(f)
                        if i >= a.warmup:
                            ms[on].append(m)
                med_off, med_on = statistics.median(ms[False]), statistics.median(ms[True])
                case = {"forward": name, "rows": int(c["x"].shape[0]), "mode": mode, "freeu_off": stats(ms[False]), "freeu_on": stats(ms[True]),
                        "on_minus_off_ms_median": round(med_on - med_off, 4), "on_over_off_median": round(med_on / med_off, 4),
                        "rel_l2_on_vs_off": round(diff, 4)}
                rec["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
            model.cache_reference = False
            model.disable_freeu()
        # the operator alone at the six (hidden, skip) shapes of one forward: up block 0 at hw / 8, up block 1 at hw / 4
        shapes = [(hw // 8, 1280, 1280)] * 3 + [(hw // 4, 1280, 1280), (hw // 4, 1280, 1280), (hw // 4, 1280, 640)]
        for B in (1, rows):
            bufs = [(torch.randn(B, n * n, C, generator=g).bfloat16().to(dev), torch.randn(B, n * n, Cs, generator=g).bfloat16().to(dev), n)
                    for n, C, Cs in shapes]
            outs = [(torch.empty_like(h), torch.empty_like(s)) for h, s, _ in bufs]

            def six():
                for (h, s, n), (ho, so) in zip(bufs, outs):
                    ops.freeu(h, s, n, n, 1.4, 0.2, hidden_out=ho, skip_out=so)
            for _ in range(a.warmup + 1):
                six()
            torch.cuda.synchronize()
            ts = [event_ms(six) for _ in range(a.iters)]
            traffic = sum(2 * (h.numel() + 1.5 * s.numel()) * 2 for h, s, _ in bufs)      # read + write; the skip map is read twice
            op = {"batch": B, "six_launches": stats(ts), "bytes_moved": int(traffic),
                  "gb_per_s_median": round(traffic / statistics.median(ts) / 1e6, 1)}
            rec["operator"].append(op)
            print(json.dumps(op), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(a.out_dir, "freeu_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
