#!/usr/bin/env python3
"""VGG-16 perceptual loss on the GPU (row N8): ``PerceptualLoss(x, y)`` of ``mvd_amd.perceptual`` at 1 and 8 pairs of 512 x 512
images in [-1, 1], He-initialised random weights.  Warm, HIP events around each call, median of the repetitions with min / max.
One JSON line per pair count to <out-dir>/perceptual_p<pairs>.json.

* ``loss``: one ``mvd_vgg_perceptual`` call (front end, 13 convolutions, 4 pools, the squared difference), in one pass;
* ``layers``: every convolution and pool of the tower on its own through the operator entry points, at the shapes the call
  runs them (2 x pairs images): ms, and TFLOP/s or GB/s from the shapes (2 M N K operations; bytes read + written);
* ``eager_bf16``: the same arithmetic as eager torch ops on the same device -- bf16 ``channels_last`` ``F.conv2d`` / ``relu`` /
  ``max_pool2d``, the last convolution's output in fp32, ``mse_loss`` -- alternating with ``loss`` in one timed window.

Needs the GPU: no fallback."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOLS_BEFORE = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)      # pools in front of each of the thirteen convolutions
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [event_ms(fn) for _ in range(iters)]


def timed_alternating(fa, fb, warmup, iters):
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(iters):
        out[0].append(event_ms(fa))
        out[1].append(event_ms(fb))
    return out


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def random_vgg(seed=0):
    import torch
    from mvd_amd.packing import VGG16_CONVS
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in VGG16_CONVS:
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
    return sd


def layer_times(packed, images, size, warmup, iters):
    """[{layer, shape, ms_median, ...}] for the convolutions (from conv1_2 on: conv1_1's im2col front end has no operator entry
    point) and the pools, on random bf16 maps"""
    import torch
    from mvd_amd import ops
    from mvd_amd.packing import VGG16_CONVS, VGG16_POOLS
    out, h = [], size
    for idx, cin, cout in VGG16_CONVS:
        if idx in (5, 10, 17, 24):
            h //= 2
        if cin == 3:
            continue
        x = torch.randn(images, h, h, cin, device="cuda").to(torch.bfloat16)
        w, b = packed[f"features.{idx}.weight"], packed[f"features.{idx}.bias"]
        last = idx == 28
        S = ops.engine_splitk(images * h * h, cout, 9 * cin, conv=True) if not last else 1
        ts = timed(lambda: ops.conv3x3_relu(x, w, b, relu=not last, out_f32=last, splitk=S), warmup, iters)
        plan = ops.last_gemm_plan()
        flop = 2.0 * images * h * h * cout * 9 * cin
        out.append(dict(stats(ts), layer=f"features.{idx}", m=images * h * h, n=cout, k=9 * cin, tile_config=plan["cfg"], splitk=plan["splitk"],
                        tflops=round(flop / statistics.median(ts) / 1e9, 1)))
        if idx + 2 in VGG16_POOLS:
            y = torch.randn(images, h, h, cout, device="cuda").to(torch.bfloat16)
            ts = timed(lambda: ops.maxpool2x2(y), warmup, iters)
            nbytes = y.numel() * 2 * 1.25
            out.append(dict(stats(ts), layer=f"features.{idx + 2} (pool)", gb_per_s=round(nbytes / statistics.median(ts) / 1e6, 1)))
    return out


def eager_tower(sd):
    import torch
    import torch.nn.functional as F
    from mvd_amd.packing import VGG16_CONVS, VGG16_POOLS
    ws = [(idx, sd[f"features.{idx}.weight"].cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last),
           sd[f"features.{idx}.bias"].cuda().to(torch.bfloat16)) for idx, _, _ in VGG16_CONVS]
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)

    def features(x):
        h = (((x + 1) / 2 - mean) / std).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        for idx, w, b in ws:
            h = F.conv2d(h, w, b, padding=1)
            if idx != 28:
                h = F.relu(h)
            if idx + 2 in VGG16_POOLS:
                h = F.max_pool2d(h, 2)
        return h.float()

    def loss(x, y):
        with torch.no_grad():
            f = features(torch.cat([x, y]))
            return F.mse_loss(f[:x.shape[0]], f[x.shape[0]:])
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,8")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-eager", action="store_true", help="this tower alone (for a run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_perceptual: needs a GPU (a CPU run measures nothing)")
    from mvd_amd.packing import VGG16_CONVS
    from mvd_amd.perceptual import PerceptualLoss
    sd = random_vgg()
    pairs_list = [int(p) for p in a.pairs.split(",")]
    loss = PerceptualLoss("cuda", weights=sd, max_pairs_per_pass=max(pairs_list))
    eager = None if a.no_eager else eager_tower(sd)
    os.makedirs(a.out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(1)
    for P in pairs_list:
        x = (torch.rand(P, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
        y = (x + 0.1 * torch.randn(P, 3, a.size, a.size, generator=g).cuda()).clamp(-1, 1).contiguous()
        run = lambda: loss(x, y)      # noqa: E731
        val = float(run())
        flop = sum(2.0 * 2 * P * (a.size >> s) ** 2 * cout * 9 * cin for (_, cin, cout), s in zip(VGG16_CONVS, POOLS_BEFORE))
        rec = {"what": f"VGG-16 perceptual loss, {P} pair(s) of {a.size} x {a.size}, random weights; warm, HIP events, one pass",
               "pairs": P, "iters": a.iters, "loss": stats(timed(run, a.warmup, a.iters)), "loss_value": val,
               "workspace_mib": round(loss.vgg._handle.ws.numel() / 2 ** 20, 1), "tower_gflop": round(flop / 1e9, 1),
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        rec["loss"]["tflops_whole_call"] = round(flop / rec["loss"]["ms_median"] / 1e9, 1)
        if not a.no_layers:
            rec["layers"] = layer_times(loss.vgg._packed, 2 * P, a.size, a.warmup, max(a.iters // 2, 5))
            rec["layers_ms_sum"] = round(sum(r["ms_median"] for r in rec["layers"]), 4)
        if eager is None:
            rec["eager_bf16"] = "skipped (--no-eager)"
        else:
            ev = float(eager(x, y))
            tl, te = timed_alternating(run, lambda: eager(x, y), a.warmup, a.iters)
            rec["loss_alternating"] = stats(tl)
            rec["eager_bf16"] = dict(stats(te), loss_value=ev, what="torch eager, bf16 channels_last conv2d / relu / max_pool2d, fp32 last map, "
                                                                   "mse_loss; alternating with loss_alternating")
            rec["speedup_over_eager_bf16_median"] = round(statistics.median(te) / statistics.median(tl), 2)
            rec["difference_beyond_spread"] = bool(abs(statistics.median(te) - statistics.median(tl)) > max(max(tl) - min(tl), max(te) - min(te)))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"perceptual_p{P}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
