#!/usr/bin/env python3
"""The device image front end (row N13) against what it replaces: ``mvd_op_image_frontend`` (composite on white + LANCZOS resize +
normalisation, two launches) for 1024 x 1024 RGBA -> 512 x 512 and 768 x 768 at batch 1, 8 and 32, and PIL's composite + resize of
ONE image on the host, single thread -- the baseline -- in the same timed window, alternating.  Warm, HIP events around the device
call (a host clock around PIL), 20 repetitions, median (min - max).

* ``device``: the call alone, the raw bytes already on the device, fp32 output;
* ``device_with_h2d``: the pinned host-to-device copy of the raw bytes in front of it, on the same stream;
* ``gb_per_s``: the bytes the two kernels must move (source read, planar uint8 intermediate written and read once, fp32 output
  written) over the device time;
* ``pil_host_per_image``: ``Image.alpha_composite(white, img).convert("RGB").resize(size, LANCZOS)`` (``null`` where PIL is absent).

One JSON line to <out-dir>/n13_frontend.json.  Nothing here assumes which side is faster.  Needs the GPU: no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_perceptual import event_ms, stats      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mvd_amd import image_frontend as F
    try:
        import PIL
        from PIL import Image
        torch.set_num_threads(1)
    except ImportError:
        PIL = Image = None
    rng = np.random.RandomState(0)
    h = w = 1024
    cases = []
    for size in (512, 768):
        pil_img = None
        if Image is not None:
            one = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
            pil_img = Image.fromarray(one, "RGBA")
            white = Image.new("RGBA", pil_img.size, (255, 255, 255, 255))

        def pil_once():
            t = time.perf_counter()
            Image.alpha_composite(white, pil_img).convert("RGB").resize((size, size), Image.Resampling.LANCZOS)
            return (time.perf_counter() - t) * 1e3
        for batch in (1, 8, 32):
            host = torch.from_numpy(rng.randint(0, 256, (batch, h, w, 4)).astype(np.uint8)).pin_memory()
            dev = host.cuda()
            call = lambda: F.composite_resize(dev, (size, size), out="float")                                   # noqa: E731
            with_copy = lambda: F.composite_resize(host.to("cuda", non_blocking=True), (size, size), out="float")   # noqa: E731
            for _ in range(a.warmup):
                call()
                with_copy()
                if pil_img is not None:
                    pil_once()
            torch.cuda.synchronize()
            t_dev, t_copy, t_pil = [], [], []
            for _ in range(a.iters):
                t_dev.append(event_ms(call))
                t_copy.append(event_ms(with_copy))
                if pil_img is not None:
                    t_pil.append(pil_once())
            ws = F.workspace_bytes(batch, h, w, 4, size, size)
            moved = batch * (h * w * 4 + 2 * 3 * h * size + 3 * size * size * 4)
            d = stats(t_dev)
            cases.append({"in": [h, w, 4], "out": [size, size], "batch": batch, "device": d, "device_with_h2d": stats(t_copy),
                          "pil_host_per_image": stats(t_pil) if t_pil else None, "bytes_moved": moved, "workspace_bytes": ws,
                          "gb_per_s": round(moved / (d["ms_median"] * 1e-3) / 1e9, 1), "device_ms_per_image": round(d["ms_median"] / batch, 4),
                          "raw_bytes_per_image": h * w * 4})
            print(cases[-1], flush=True)
    out = {"what": "mvd_op_image_frontend (composite on white, LANCZOS, / 127.5 - 1) on 1024 x 1024 RGBA, fp32 output; warm, HIP events; "
                   "PIL composite + resize of one image on the host (single thread, host clock), alternating in the same window",
           "iters": a.iters, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pillow": PIL.__version__ if PIL else None,
           "spans": F.spans(), "cases": cases}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "n13_frontend.json"), "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
