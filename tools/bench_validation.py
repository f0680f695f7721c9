#!/usr/bin/env python3
"""Checkpoint scoring: the fused kernels of csrc/losses.hip against THE SAME arithmetic composed from PyTorch-ROCm eager ops on
the same device, in one process, alternating the two, warm, HIP events around each call, median of >= 20 repetitions with
min / max.  One JSON line per case to <out-dir>/validation_<case>.json.

Cases: ``noise_loss_b32`` -- the noise-loss part of ``compute_losses`` (v_prediction target, denoised latents, both squared
errors, the Min-SNR weights) at (32, 4, 64, 64); ``image_metrics_32x512`` / ``image_metrics_8x768`` -- MSE + SSIM of
32 x 3 x 512 x 512 and 8 x 3 x 768 x 768.  A fused path counts as faster only when the medians differ by more than the
min-max spread of its own repetitions (``faster_beyond_spread``).

Kernel time (not call time) comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir>/<case> -- python tools/bench_validation.py --profile-run --case <case>
    python tools/bench_validation.py --stats-dir <dir>            # the timed run; merges <dir>/<case>/**/*kernel_stats.csv

and is reported next to the algorithmic bytes (every input read once, every output written once; the record also holds the
figure with each input counted twice) as a bandwidth and as a share of the 6.3 TB/s that elementwise kernels reach on this part
(MI355X_MICROARCH.md: measured float4 copy).  Needs the GPU: no fallback.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ELEMENTWISE = 6.3e12
CASES = ("noise_loss_b32", "image_metrics_32x512", "image_metrics_8x768")
MAIN_KERNEL = {"noise_loss_b32": "noise_loss_kernel", "image_metrics_32x512": "ssim_tile_kernel", "image_metrics_8x768": "ssim_tile_kernel"}


def make_case(name):
    """-> (fused(), eager(), algorithmic bytes read, written)"""
    import torch
    import torch.nn.functional as F
    from mvd_amd import ops, validation as V
    from mvd_amd.pipeline import _make_scheduler
    g = torch.Generator().manual_seed(0)
    if name == "noise_loss_b32":
        sched = _make_scheduler(None, "ddpm")
        a, s = sched.noise_tables("cuda:0")
        snr = V.snr_table(sched, "cuda:0")
        shape = (32, 4, 64, 64)
        pred, eps, x0 = (torch.randn(shape, generator=g).cuda() for _ in range(3))
        ts = torch.randint(0, 1000, (32,), generator=g).cuda()
        noisy = sched.add_noise(x0, eps, ts)

        def fused():
            return ops.noise_loss(pred, eps, ts, a, s, snr, "v_prediction", x0=x0, noisy=noisy, want_denoised=True)

        def eager():
            at, st = a[ts].view(-1, 1, 1, 1), s[ts].view(-1, 1, 1, 1)
            target = at * eps - st * x0
            mse = F.mse_loss(pred, target)
            r = snr[ts]
            w = torch.minimum(r, torch.full_like(r, 5.0)) / r
            den = at * noisy - st * pred
            return torch.stack([mse, mse * w.mean(), F.mse_loss(den, x0), r.mean(), w.mean()]), den
        n = pred.numel() * 4
        return fused, eager, 4 * n, n
    n_img, hw = (32, 512) if name == "image_metrics_32x512" else (8, 768)
    x = torch.rand(n_img, 3, hw, hw, generator=g).cuda() * 2 - 1
    y = (x + 0.05 * torch.randn(n_img, 3, hw, hw, generator=g).cuda()).contiguous()
    win = torch.exp(-((torch.arange(11, dtype=torch.float32) - 5) ** 2) / (2 * 1.5 ** 2))
    win = (win / win.sum()).cuda()
    wv, wh = win.view(1, 1, 11, 1).repeat(3, 1, 1, 1), win.view(1, 1, 1, 11).repeat(3, 1, 1, 1)
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2

    def filt(t):
        return F.conv2d(F.conv2d(t, wv, groups=3), wh, groups=3)

    def fused():
        return ops.image_metrics(x, y, 2.0, ssim=True)

    def eager():             # pytorch_msssim's own sequence of ops
        mu1, mu2 = filt(x), filt(y)
        mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s11, s22, s12 = filt(x * x) - mu1_sq, filt(y * y) - mu2_sq, filt(x * y) - mu12
        cs = (2 * s12 + c2) / (s11 + s22 + c2)
        ssim = (((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs).flatten(2).mean(-1).mean()
        mse = F.mse_loss(x, y)
        return torch.stack([mse, ssim, 10 * torch.log10(4.0 / mse)])
    n = x.numel() * 4
    return fused, eager, 2 * n, 0


def timed_alternating(fa, fb, warmup, iters):
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(iters):
        for k, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def kernel_stats(stats_dir, case):
    """{kernel name: (calls, average ns)} of the case's profiler run, or None."""
    files = glob.glob(os.path.join(stats_dir, case, "**", "*kernel_stats.csv"), recursive=True) if stats_dir else []
    if not files:
        return None
    out = {}
    with open(sorted(files)[-1]) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=",".join(CASES))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats-dir", default=None, help="directory holding <case>/**/*kernel_stats.csv of the profiler runs")
    ap.add_argument("--profile-run", action="store_true", help="only launch the fused path (for a run under rocprofv3)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_validation: needs a GPU (a CPU run measures nothing)")
    os.makedirs(a.out_dir, exist_ok=True)
    for case in a.case.split(","):
        fused, eager, rd, wr = make_case(case)
        if a.profile_run:
            for _ in range(a.warmup + max(a.iters, 20)):
                fused()
            torch.cuda.synchronize()
            continue
        rf, re_ = fused(), eager()
        torch.cuda.synchronize()
        agree = max(abs(float(p) - float(q)) / max(abs(float(q)), 1e-30) for p, q in zip(rf[0].tolist(), (re_[0] if isinstance(re_, tuple) else re_).tolist()))
        tf, te = timed_alternating(fused, eager, a.warmup, max(a.iters, 20))
        mf, me = statistics.median(tf), statistics.median(te)
        rec = {"what": f"{case}: fused HIP kernels vs the same arithmetic in PyTorch-ROCm eager ops, alternating, HIP events, warm",
               "iters": len(tf), "fused_ms_median": round(mf, 4), "fused_ms_min": round(min(tf), 4), "fused_ms_max": round(max(tf), 4),
               "eager_ms_median": round(me, 4), "eager_ms_min": round(min(te), 4), "eager_ms_max": round(max(te), 4),
               "speedup_median": round(me / mf, 2), "faster_beyond_spread": bool(me - mf > max(tf) - min(tf)),
               "max_relative_difference_of_results": agree,
               "algorithmic_bytes": rd + wr, "algorithmic_bytes_inputs_counted_twice": 2 * rd + wr,
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        st = kernel_stats(a.stats_dir, case)
        if st is None:
            rec["kernel_time"] = "not measured (no profiler run given)"
        else:
            main_k = [(n, v) for n, v in st.items() if MAIN_KERNEL[case] in n]
            rec["kernels"] = {n: {"calls": c, "avg_us": round(ns / 1e3, 3)} for n, (c, ns) in st.items()
                              if "losses" in n or "kernel" in n and any(k in n for k in ("noise_loss", "ssim_tile", "image_metrics", "sqdiff"))}
            if main_k:
                ns = main_k[0][1][1]
                bw = (rd + wr) / (ns * 1e-9)
                rec.update({"main_kernel": main_k[0][0], "main_kernel_avg_us": round(ns / 1e3, 3),
                            "algorithmic_TBs": round(bw / 1e12, 3), "share_of_6.3TBs_elementwise": round(bw / HBM_ELEMENTWISE, 3),
                            "algorithmic_TBs_inputs_counted_twice": round((2 * rd + wr) / (ns * 1e-9) / 1e12, 3)})
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"validation_{case}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
