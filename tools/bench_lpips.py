#!/usr/bin/env python3
"""LPIPS on the GPU (row N9): ``LPIPS(net)(x, y)`` of ``mvd_amd.lpips`` for ``alex`` and ``vgg`` at 1 and 8 pairs of 512 x 512
images in [-1, 1], He-initialised random backbones and |N(0, 1)| / C linear heads.  Warm, HIP events around each call, median of
the repetitions with min / max.  One JSON line per (net, pair count) to <out-dir>/lpips_<net>_p<pairs>.json.

* ``distance``: one call of the metric -- for ``alex`` one ``mvd_lpips_distance`` (2 im2col, 5 GEMMs and their split-K reduce
  passes, 2 pools, the head and its finish), for ``vgg`` ``mvd_vgg_features`` with its taps plus ``mvd_op_lpips_head`` -- in one pass;
* ``eager_bf16``: the same arithmetic as eager torch ops on the same device -- bf16 ``channels_last`` ``F.conv2d`` / ``relu`` /
  ``max_pool2d``, the head in fp32 -- alternating with ``distance`` in one timed window.  For ``vgg`` the eager fifth tap is a
  bf16 map, while this project's path keeps ``features.28`` in fp32: the same work for a timing, not the same bits.

Needs the GPU: no fallback."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import random_vgg, stats, timed, timed_alternating      # noqa: E402


def random_alex(seed=0):
    import torch
    from mvd_amd.packing import ALEX_CONVS
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout, k, _, _ in ALEX_CONVS:
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (k * k * cin))
        sd[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
    return sd


def random_lins(channels, seed=0):
    import torch
    g = torch.Generator().manual_seed(100 + seed)
    return {f"lin{k}.model.1.weight": (torch.randn(c, generator=g).abs() / c).reshape(1, c, 1, 1) for k, c in enumerate(channels)}


def eager_metric(net, sd, lins):
    import torch
    import torch.nn.functional as F
    from mvd_amd.packing import ALEX_CONVS, ALEX_POOLS, LPIPS_SCALE, LPIPS_SHIFT, VGG16_CONVS, VGG16_POOLS
    convs = [(c[0], c[4], c[5]) for c in ALEX_CONVS] if net == "alex" else [(c[0], 1, 1) for c in VGG16_CONVS]
    pools, pool_k = (ALEX_POOLS, (3, 2)) if net == "alex" else (VGG16_POOLS, (2, 2))
    taps_at = (0, 3, 6, 8, 10) if net == "alex" else (2, 7, 14, 21, 28)
    ws = [(idx, s, p, sd[f"features.{idx}.weight"].cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last),
           sd[f"features.{idx}.bias"].cuda().to(torch.bfloat16)) for idx, s, p in convs]
    lw = [lins[f"lin{k}.model.1.weight"].cuda().float() for k in range(5)]
    shift = torch.tensor(LPIPS_SHIFT, device="cuda").view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, device="cuda").view(1, 3, 1, 1)

    def metric(x, y):
        with torch.no_grad():
            n = x.shape[0]
            h = ((torch.cat([x, y]) - shift) / scale).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            d = 0
            for idx, s, p, w, b in ws:
                h = F.relu(F.conv2d(h, w, b, stride=s, padding=p))
                if idx in taps_at:
                    f = h.float()
                    f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                    d = d + (lw[taps_at.index(idx)] * (f[:n] - f[n:]).pow(2)).sum(1, keepdim=True).mean((2, 3), keepdim=True)
                if idx + 2 in pools:
                    h = F.max_pool2d(h, *pool_k)
            return d
    return metric


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="alex,vgg")
    ap.add_argument("--pairs", default="1,8")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-eager", action="store_true", help="this path alone (for a run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lpips: needs a GPU (a CPU run measures nothing)")
    from mvd_amd.lpips import LPIPS, TAP_CHANNELS
    pairs_list = [int(p) for p in a.pairs.split(",")]
    os.makedirs(a.out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(1)
    for net in a.nets.split(","):
        sd, lins = (random_alex() if net == "alex" else random_vgg()), random_lins(TAP_CHANNELS[net])
        metric = LPIPS(net=net, backbone=sd, model_path=lins, max_pairs_per_pass=max(pairs_list))
        eager = None if a.no_eager else eager_metric(net, sd, lins)
        for P in pairs_list:
            x = (torch.rand(P, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
            y = (x + 0.1 * torch.randn(P, 3, a.size, a.size, generator=g).cuda()).clamp(-1, 1).contiguous()
            run = lambda: metric(x, y)      # noqa: E731
            val = run().reshape(-1).tolist()
            rec = {"what": f"LPIPS({net}), {P} pair(s) of {a.size} x {a.size}, random weights; warm, HIP events, one pass",
                   "net": net, "pairs": P, "iters": a.iters, "distance": stats(timed(run, a.warmup, a.iters)), "distance_values": val,
                   "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
            if net == "alex":
                rec["workspace_mib"] = round(metric._handle.ws.numel() / 2 ** 20, 1)
            if eager is None:
                rec["eager_bf16"] = "skipped (--no-eager)"
            else:
                ev = eager(x, y).reshape(-1).tolist()
                tl, te = timed_alternating(run, lambda: eager(x, y), a.warmup, a.iters)
                rec["distance_alternating"] = stats(tl)
                rec["eager_bf16"] = dict(stats(te), distance_values=ev, what="torch eager, bf16 channels_last conv2d / relu / max_pool2d, the head "
                                                                             "in fp32; alternating with distance_alternating"
                                                                             + ("; its fifth tap is a bf16 map, where this project's path keeps "
                                                                                "features.28 in fp32" if net == "vgg" else ""))
                rec["speedup_over_eager_bf16_median"] = round(statistics.median(te) / statistics.median(tl), 2)
                rec["difference_beyond_spread"] = bool(abs(statistics.median(te) - statistics.median(tl)) > max(max(tl) - min(tl), max(te) - min(te)))
            line = json.dumps(rec)
            print(line, flush=True)
            with open(os.path.join(a.out_dir, f"lpips_{net}_p{P}.json"), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
