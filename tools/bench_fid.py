#!/usr/bin/env python3
"""FID on the GPU (row N10): ``FrechetInceptionDistance.update`` of ``mvd_amd.fid`` at 1 and 8 uint8 images of 512 x 512,
He-initialised random weights (BatchNorm folded).  Warm, HIP events around each call, median of the repetitions with min / max.
One JSON line per image count to <out-dir>/fid_p<images>.json.

* ``update``: one call -- ``mvd_fid_update``: the front end, 94 convolutions and 13 pools, the mean, the two statistics kernels;
* ``features``: ``mvd_fid_features`` alone (no statistics);
* ``blocks``: the same operators launched one by one through ``mvd_amd.ops`` over the layer table, HIP events around each block
  (the stem, Mixed_5b ... Mixed_7c); the Python launch overhead of the one-by-one replay is inside these figures, so their sum
  exceeds ``features``;
* ``eager_bf16``: the same arithmetic as eager torch ops on the same device -- bf16 ``channels_last`` ``F.conv2d`` / ``relu`` /
  ``avg_pool2d`` / ``max_pool2d`` into slices of preallocated concatenation buffers, ``F.interpolate`` in front (torch's bilinear
  resize, not the TF1-legacy one: the same work for a timing, not the same bits), the statistics as fp64 ``f.T @ f`` --
  alternating with ``update`` in one timed window.

Needs the GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_perceptual import stats, timed, timed_alternating      # noqa: E402


def block_of(dst):
    name = dst.split(".")[0]
    return name if name.startswith("Mixed") else "stem"


def block_times(packed, images, warmup, iters):
    """[{block, ms_median, ...}]: the table replayed operator by operator on the buffers of one pass"""
    import torch
    from mvd_amd import ops
    from mvd_amd import packing as P
    ch, hw = P.fid_buffer_channels(), P.fid_geometry()
    ch["img"] = P.FID_INPUT_CHANNELS
    n = images.shape[0]
    bufs = {k: torch.empty(n, hw[k][0], hw[k][1], c, device="cuda", dtype=torch.float32 if k == P.FID_FEATURE_BUFFER else torch.bfloat16)
            for k, c in ch.items()}
    bufs["img"] = ops.resize_tf1(images)
    groups = {}
    for e in P.INCEPTION_FID_LAYERS:
        groups.setdefault(block_of(e[3]), []).append(e)

    def run_block(entries):
        for e in entries:
            if e[0] == "conv":
                _, name, src, dst, c_off, _, _, kh, kw, s, ph, pw = e
                ops.conv_relu_slice(bufs[src], packed[f"{name}.weight"], packed[f"{name}.bias"], kh, kw, s, (ph, pw), out=bufs[dst], c_off=c_off,
                                    out_f32=dst == P.FID_FEATURE_BUFFER)
            else:
                ops.pool3x3_slice(bufs[e[2]], e[1], out=bufs[e[3]], c_off=e[4])
    out = []
    for blk, entries in groups.items():
        ts = timed(lambda: run_block(entries), warmup, iters)
        out.append(dict(block=blk, operators=len(entries), **stats(ts)))
    return out


def eager_update(sd):
    import torch
    import torch.nn.functional as F
    from mvd_amd import packing as P
    folded = {n: (w.cuda().contiguous(memory_format=torch.channels_last), b.cuda().to(torch.bfloat16)) for n, (w, b) in P.fold_inception_fid(sd).items()}
    ch, hw = P.fid_buffer_channels(), P.fid_geometry()
    total = torch.zeros(2048, dtype=torch.float64, device="cuda")
    cov = torch.zeros(2048, 2048, dtype=torch.float64, device="cuda")

    def update(images):
        with torch.no_grad():
            n = images.shape[0]
            x = F.interpolate(images.float(), size=(P.FID_INPUT_SIZE, P.FID_INPUT_SIZE), mode="bilinear", align_corners=False)
            bufs = {"img": ((x - 128.0) / 128.0).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)}
            for e in P.INCEPTION_FID_LAYERS:
                src = bufs[e[2]]
                if e[0] == "conv":
                    _, name, _, dst, c_off, _, cout, _, _, s, ph, pw = e
                    y = F.relu(F.conv2d(src, *folded[name], stride=s, padding=(ph, pw)))
                else:
                    _, mode, _, dst, c_off, cout = e
                    y = (F.avg_pool2d(src, 3, 1, 1, count_include_pad=False) if mode == "avg" else F.max_pool2d(src, 3, 1, 1) if mode == "max1"
                         else F.max_pool2d(src, 3, 2))
                if dst not in bufs:
                    bufs[dst] = torch.empty(n, ch[dst], *hw[dst], device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
                bufs[dst][:, c_off:c_off + cout] = y
            f = bufs[P.FID_FEATURE_BUFFER].float().mean((2, 3)).double()
            total.add_(f.sum(0))
            cov.add_(f.t() @ f)
            return f
    return update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default="1,8")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-eager", action="store_true", help="this path alone (for a run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fid: needs a GPU (a CPU run measures nothing)")
    import fid_ref
    from mvd_amd.fid import FrechetInceptionDistance
    counts = [int(p) for p in a.images.split(",")]
    os.makedirs(a.out_dir, exist_ok=True)
    sd = fid_ref.synthetic_inception_state_dict(0)
    metric = FrechetInceptionDistance(weights=sd, max_images_per_pass=max(counts))
    eager = None if a.no_eager else eager_update(sd)
    g = torch.Generator().manual_seed(1)
    for n in counts:
        x = torch.randint(0, 256, (n, 3, a.size, a.size), generator=g, dtype=torch.uint8).cuda()
        run = lambda: metric.update(x, real=True)      # noqa: E731
        run()
        rec = {"what": f"FrechetInceptionDistance.update, {n} image(s) of {a.size} x {a.size} uint8, random weights; warm, HIP events, one pass",
               "images": n, "iters": a.iters, "update": stats(timed(run, a.warmup, a.iters)),
               "features": stats(timed(lambda: metric.inception(x), a.warmup, a.iters)),
               "blocks": block_times(metric.inception._packed, x, a.warmup, a.iters),
               "workspace_mib": round(metric.inception._handle.ws.numel() / 2 ** 20, 1),
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        if eager is None:
            rec["eager_bf16"] = "skipped (--no-eager)"
        else:
            fe, fo = eager(x).float(), metric.inception(x)
            rec["eager_features_rel_l2"] = float((fe - fo).norm() / fo.norm())
            tl, te = timed_alternating(run, lambda: eager(x), a.warmup, a.iters)
            rec["update_alternating"] = stats(tl)
            rec["eager_bf16"] = dict(stats(te), what="torch eager, bf16 channels_last conv2d / relu / pools into slices, F.interpolate in front, "
                                                     "fp64 f.T @ f; alternating with update_alternating")
            rec["speedup_over_eager_bf16_median"] = round(statistics.median(te) / statistics.median(tl), 2)
            rec["difference_beyond_spread"] = bool(abs(statistics.median(te) - statistics.median(tl)) > max(max(tl) - min(tl), max(te) - min(te)))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"fid_p{n}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
