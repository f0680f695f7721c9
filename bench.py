#!/usr/bin/env python3
"""Headline benchmark: UNet forward-passes/sec at 512x512 (64x64x4 latent, 77 text tokens) for the
SD-2.1 UNet + MVD camera/cross-view adapter hot path on MI355X.

    python bench.py --gpus 1 --steps K --warmup W            (single GPU)
    python bench.py --gpus N --steps K --warmup W            (starts N ranks itself: the parent never touches a GPU,
                                                              it runs torch.distributed.run as a child and relays rank 0's line)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (one rank per GPU, launcher form)

A "step" is one ``MultiViewUNet.forward`` over one batch of synthetic (source -> target) pairs that
is already resident in HBM.  The default workload is BASELINE.json configs[3] per GPU (8 objects x 4
target views = 32 pairs, camera + image conditioning on); configs[4] is that shard on each of N GPUs
(weak scaling; the only collective is the start-up RCCL weight broadcast).  By default the forward
is reference-faithful ("cold"): the frozen reference-image UNet is re-run every step exactly as
/root/reference/src/models/mvd_unet.py:287-291 does; ``--cached`` reuses its step-invariant K/V (Q5).

Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the ``--steps`` forwards and prints the line (``value``, ``ms_per_step``).  Everything
else it can measure or check -- the determinism / cross-path output screens, the per-kernel-class profile and roofline, the
CPU baseline, the attention-statistics proxy, e2e's per-phase times -- runs only with ``--full`` (each still switched off by
its own ``--no-*`` option there).  ``--dump-outputs DIR`` writes what the last timed step returned as ``DIR/<name>.npy``.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# algorithmic FLOPs per (source -> target) pair per forward (2*MAC over convs, linears, QK^T/PV): SURVEY.md 8d
F_BASE, F_ADAPTER_MAIN, F_ENCODER = 804.26e9, 1151.59e9, 804.26e9


def unet_flops(H: int, W: int, L: int = 77, adapter: bool = False, xd: int = 1024) -> float:
    """SURVEY.md 8d's count for any latent size: 2*MAC over convs, linears and QK^T / PV of the SD-2.1 topology (norms,
    activations, softmax excluded); ``adapter`` adds the cross-view branch of all 16 transformer sites (q_ref, attention
    over the reference tokens, to_out_ref, K_ref / V_ref projections).  64 x 64: 804.26 / 1151.59 GFLOP (the SURVEY's
    figures); 96 x 96 (768^2 images): 2149.11 / 3619.63 GFLOP."""
    ch, n, Lb = [320, 640, 1280, 1280], 4, 2
    fl = 2 * H * W * 320 * 36 + 2 * (320 * 1280 + 1280 * 1280) + 2 * H * W * 4 * 9 * 320

    def resnet(ci, co, hw):
        return 2 * hw * co * 9 * ci + 2 * hw * co * 9 * co + 2 * 1280 * co + (2 * hw * co * ci if ci != co else 0)

    def tr(C, hw):
        f = 40 * hw * C * C + 4 * hw * hw * C + 4 * hw * L * C + 4 * L * xd * C
        return f + (16 * hw * C * C + 8 * hw * hw * C if adapter else 0)

    h, w, prev, skips = H, W, 320, [320]
    for i in range(n):
        co = ch[i]
        for j in range(Lb):
            fl += resnet(prev if j == 0 else co, co, h * w) + (tr(co, h * w) if i < n - 1 else 0)
            skips.append(co)
        prev = co
        if i < n - 1:
            h, w = h // 2, w // 2
            fl += 2 * h * w * co * 9 * co
            skips.append(co)
    fl += 2 * resnet(1280, 1280, h * w) + tr(1280, h * w)
    prev_out = 1280
    for i in range(n):
        co = ch[n - 1 - i]
        for j in range(Lb + 1):
            fl += resnet((prev_out if j == 0 else co) + skips.pop(), co, h * w) + (tr(co, h * w) if i > 0 else 0)
        prev_out = co
        if i < n - 1:
            h, w = 2 * h, 2 * w
            fl += 2 * h * w * co * 9 * co
    return float(fl)
PEAK_BF16_MFMA = 2.5e15          # dense, /opt/skills/guides/MI355X_MICROARCH.md:43
PEAK_HBM = 8.0e12

WORKLOADS = {
    # name: (pairs per GPU, camera, image conditioning, description)
    "cfg4": (32, True, True, "configs[3]/[4]: 8 objects x 4 target views per GPU (32 pairs), camera FiLM + cross-view adapter"),
    "cfg3": (1, True, True, "configs[2]: 1 source -> 1 target view, camera FiLM + cross-view adapter"),
    "cfg2": (1, False, False, "configs[1]: base SD2.1 UNet, batch 1, both conditionings off"),
}


def fill_synthetic_weights(model, seed: int = 0, q_scale: float = 1.0):
    """Seeded variance-preserving random weights directly on the GPU (no pretrained SD-2.1 weights exist offline).
    ``q_scale`` multiplies every query projection (to_q / to_q_ref): variance-preserving weights give attention logits of
    unit spread, i.e. nearly FLAT softmaxes over 4096 keys -- a trained checkpoint's are peaked (``--attn-stats peaked``)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g, device="cuda") / math.sqrt(fan_in))
                if q_scale != 1.0 and (name.endswith("to_q.weight") or name.endswith("to_q_ref.weight")):
                    p.mul_(q_scale)
            elif name.endswith("weight"):      # every 1-D weight is a GroupNorm / LayerNorm scale
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g, device="cuda"))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g, device="cuda"))
    model.mark_weights_changed()


def softmax_stats_proxy(q_scale: float, keys: int = 4096, C: int = 320, heads: int = 5, seed: int = 3):
    """What ``q_scale`` does to a self-attention row of the 64x64 level, measured (torch, measurement glue only) on LayerNorm-like
    inputs (unit-variance rows) through variance-preserving to_q / to_k of the synthetic initialisation: entropy of a row's
    softmax over ``keys`` keys and the probability mass of its 8 largest entries, averaged over 256 sampled queries x heads."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.randn(keys, C, generator=g, device="cuda")
    wq = torch.randn(C, C, generator=g, device="cuda") / math.sqrt(C) * q_scale
    wk = torch.randn(C, C, generator=g, device="cuda") / math.sqrt(C)
    q = (h[:256] @ wq.T).reshape(256, heads, C // heads).transpose(0, 1)
    k = (h @ wk.T).reshape(keys, heads, C // heads).transpose(0, 1)
    p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C // heads), dim=-1)
    ent = -(p * p.clamp_min(1e-30).log()).sum(-1).mean().item()
    top8 = p.topk(8, dim=-1).values.sum(-1).mean().item()
    return {"q_scale": q_scale, "entropy_nats": round(ent, 3), "uniform_entropy_nats": round(math.log(keys), 3), "top8_mass": round(top8, 4),
            "measured_on": f"{keys} unit-variance key rows, 256 queries x {heads} heads, variance-preserving to_q / to_k (torch)"}


def make_batch(pairs: int, rank: int, device, lat_hw: int = 64):
    """8 objects x 4 target views per 32 pairs.  As pipeline.py:111-116 does, each object's source IMAGE (and prompt) is
    repeated per view, and ``latent_dist.sample()`` then draws a separate latent per ROW: the text rows repeat 4x, the
    32 source latents are distinct (a shared per-object mean plus per-row posterior noise).  The engine makes no use of
    any repetition."""
    from mvd_amd.utils import look_at
    g = torch.Generator().manual_seed(1000 + rank)
    objs = max(1, pairs // 4)
    views = pairs // objs
    sample = torch.randn(pairs, 4, lat_hw, lat_hw, generator=g)
    text = torch.randn(objs, 77, 1024, generator=g).repeat_interleave(views, 0)
    mean = torch.randn(objs, 4, lat_hw, lat_hw, generator=g).repeat_interleave(views, 0)      # pipeline.py:111-113
    lat = 0.18215 * (mean + 0.1 * torch.randn(pairs, 4, lat_hw, lat_hw, generator=g))          # pipeline.py:115-116
    src = torch.stack([look_at(0.0)] * pairs)
    tgt = torch.stack([look_at([45.0, 90.0, 180.0, 270.0][i % 4]) for i in range(pairs)])
    t = torch.full((pairs,), 500.0)
    return {k: v.to(device).contiguous() for k, v in dict(sample=sample, text=text, lat=lat, src=src, tgt=tgt, t=t).items()}


# --dump-outputs: at most this many bytes of .npy files in all; the per-call random draws of the timed path (Q1's Fourier
# projection, e2e's initial noise and posterior samples) come from torch's default generators, seeded with this before warm-up
DUMP_BYTES_MAX = 64 << 20
OUTPUT_SEED = 20240


def dump_outputs(outdir: str, arrays: dict, budget: int = DUMP_BYTES_MAX) -> dict:
    """Write each tensor as ``outdir/<name>.npy`` in float32, in its own shape.  A tensor larger than its share of ``budget``
    is replaced by a fixed, seeded sample of its flattened elements (sorted indices, the same for the same shape), stored 1-D.
    -> {name: [shape written, elements of the full output]}."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    share = budget // max(1, len(arrays)) - 4096          # (room for the .npy header)
    written = {}
    for name, t in arrays.items():
        a = t.detach().float().cpu()
        full = a.numel()
        if full * 4 > share:
            g = torch.Generator().manual_seed(OUTPUT_SEED)
            idx = torch.randint(0, full, (share // 4,), generator=g).sort().values
            a = a.flatten()[idx]
        np.save(os.path.join(outdir, f"{name}.npy"), a.numpy())
        written[name] = [list(a.shape), full]
    return written


def cpu_baseline(timed_runs: int = 3, warmup_runs: int = 1, latent: int = 64):
    """The oracle (CPU fp32 restatement, oracle/mvd.py) timed on this box's host cores: configs[2] (B=1, adapter + camera
    on, cold forward; 13-16 s per forward with torch's default 128 threads on the GPU box, whose cgroup grants 16 cores -- hence
    ``oracle.host_threads()``).  BASELINE.md section 3 protocol: 1 warm-up forward, then ``timed_runs`` timed ones, MEDIAN reported.  The only place bench.py
    touches ``oracle/`` (and tests/parity_util, which imports it)."""
    import statistics
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs
    # the threads the box can actually run: torch's default capped by the cgroup CPU quota (16 cores on the pool's one-GPU boxes,
    # where os.cpu_count() and the affinity mask show all 256 hardware threads and torch defaults to 128 -- 128 threads on a
    # 16-core quota run this forward 3.9x slower than 16 do, profiles/r04_probe_oracle_threads.log)
    import oracle
    default_threads = torch.get_num_threads()
    cores = oracle.host_threads()
    torch.set_num_threads(cores)
    cfg = OU.UNetConfig.sd21()
    params = OM.init_mvd_params(cfg, 0, share_encoder=True)
    inp = make_inputs(cfg, 1, latent, 77, 0, 1024)
    times = []
    with torch.no_grad():
        for i in range(warmup_runs + timed_runs):
            t0 = time.perf_counter()
            OM.multiview_unet_forward(params, cfg, inp["sample"], torch.tensor(500), inp["text"], inp["src"], inp["tgt"],
                                      inp["lat"], fourier_proj=inp["proj"])
            if i >= warmup_runs:
                times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    torch.set_num_threads(default_threads)
    return {"value": 1.0 / med, "unit": "forward-passes/s", "cores": cores, "kind": "port",
            "sample": f"oracle/mvd.py, configs[2] (B=1, {latent}x{latent} latent, adapter+camera on, cold forward = "
                      f"{(unet_flops(latent, latent, adapter=True) + unet_flops(latent, latent)) / 1e9:.0f} GFLOP), "
                      f"{warmup_runs} warm-up + {timed_runs} timed forwards (median; min {min(times):.2f} s, max {max(times):.2f} s), "
                      f"torch fp32 on {cores} host threads (torch default {default_threads}, os.cpu_count()={os.cpu_count()}; "
                      f"capped by the cgroup CPU quota), {med:.2f} s/forward"}


def _strip_comments(src: str) -> str:
    """Drop // and /* */ comments, blank lines and leading / trailing white space (string literals in the kernels never
    contain comment markers): what remains decides the generated code."""
    import re
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = []
    for line in src.splitlines():
        line = re.sub(r"//.*$", "", line).strip()
        if line:
            out.append(line)
    return "\n".join(out)


def kernel_source_sha(read=None) -> str:
    """Hash of the HIP sources + headers the library is built from (comments and blank lines excluded) and of the hipcc flags: PMC summaries under
    profiles/ are stamped with it, and ``roofline.traffic`` is only quoted from a summary taken on THIS code state.
    ``read(path) -> str`` lets a tool hash another revision of the same files."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "mvd_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            path = os.path.join(d, f)
            text = read(path) if read else open(path, "r").read()
            h.update(f.encode())
            h.update(_strip_comments(text).encode())
    from mvd_amd import _build
    h.update(" ".join(_build.FLAGS).encode())          # a change of code-generation flags is a change of kernels
    return h.hexdigest()[:16]


def output_check(model, batch, kw, step, strict_cross: bool = True):
    """Cheap screens on the numbers the timed kernels produce (the parity proper is tests/test_cfg4_shapes_gpu.py):
    (a) two forwards of the same batch with the Fourier projection pinned are BIT-identical (race / uninitialised-read
    screen on the persistent multi-tile kernels); (b) with image conditioning off (no batch coupling, Q2) rows 0-1 of
    the full-batch forward equal a batch-2 forward of the same rows -- computed by different tile configurations and
    grids -- to bf16 accumulation-order noise."""
    keep = model.fourier_projection
    if model.camera_encoder is not None:      # a fixed projection for the screen (the timed steps draw a fresh one per call, Q1)
        g = torch.Generator().manual_seed(4321)
        enc_dim = 6 * model.camera_encoder.pos_enc_dim
        model.fourier_projection = (torch.randn(model.camera_encoder.output_dim, enc_dim, generator=g) / math.sqrt(enc_dim)).to(batch["sample"].device)
    f0, a, b = step().clone(), step().clone(), step().clone()      # three forwards: a first-call effect shows as f0 != a == b
    res = {"deterministic": bool(torch.equal(a, b)) and bool(torch.equal(f0, a))}
    if not res["deterministic"]:
        if torch.equal(a, b):
            a = f0
        sys.stderr.write(f"determinism screen: forward 0 == 1: {bool(torch.equal(f0, a))}, 1 == 2: {bool(torch.equal(a, b))}, 0 == 2: {bool(torch.equal(f0, b))}\n")
        d = (a.float() - b.float()).abs()
        bad = (a != b)
        rows = bad.flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"two forwards of the same inputs differ: {int(bad.sum())} of {a.numel()} elements, max |diff| "
                             f"{float(torch.nan_to_num(d, nan=-1.0).max()):.3e}, NaNs {int(torch.isnan(a).sum())}/{int(torch.isnan(b).sum())}, "
                             f"batch rows {rows[:12]}, (b, c, y, x) of the first: {bad.nonzero()[:8].tolist()}, "
                             f"a/b there: {a[bad][:8].tolist()} / {b[bad][:8].tolist()}")
    cam = {k: v for k, v in kw.items() if k != "source_image_latents"}
    if batch["sample"].shape[0] >= 4:
        with torch.no_grad():
            full = model(batch["sample"], batch["t"], batch["text"], **cam).sample[:2]
            small = model(batch["sample"][:2], batch["t"][:2], batch["text"][:2], **{k: v[:2] for k, v in cam.items()}).sample
        rel = ((full - small).norm() / small.norm()).item()
        res["full_batch_vs_batch2_rel_l2"] = round(rel, 6)
        # two bf16 evaluations of ~300 chained ops each sit ~1e-2 from the fp32 truth (tests/test_cfg4_shapes_gpu.py); a wrong
        # tile or a race shows up as O(1)
        # (--attn-stats peaked: random weights with logits of spread ~8 make the 16-layer network chaotic -- a bf16 rounding of a
        #  score moves whole probability masses -- so two correct evaluations through different tile shapes no longer agree; the
        #  number is reported, not asserted.  Bit-determinism above still holds and still screens races.)
        assert rel <= 3e-2 or not strict_cross, f"full-batch rows differ from their batch-2 recomputation: rel-L2 {rel}"
    model.fourier_projection = keep
    return res


def e2e_workload(args, dev):
    """BASELINE's metric is the UNet forward; the one number the reference itself measures is seconds per generated image
    (/root/reference/val.py:331-347).  This workload times what infer.py:111-122 runs for ONE image: VAE encode of the source
    image -> N-step denoising loop (B = 1, guidance 1.0, camera + image conditioning) -> VAE decode, through
    ``MVDPipeline.__call__``, synthetic weights of the SD-2.1 shapes.  ``--cached`` = cache_reference (Q5)."""
    import statistics
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    from mvd_amd.pipeline import MVDPipeline
    from mvd_amd.scheduler import DDPMScheduler, ShiftSNRScheduler
    from mvd_amd.utils import look_at
    from mvd_amd.vae import AutoencoderKLHIP
    L_ = args.latent
    model = MultiViewUNet(None, unet_config=UNetConfig.sd21(), init="empty", img_ref_scale=0.25, cam_modulation_strength=1.0,
                          cache_reference=args.cached, dedup_encoder_weights=False).to(dev)
    model.eval()
    fill_synthetic_weights(model, 0)
    model._sync_engine()
    torch.manual_seed(1)
    vae = AutoencoderKLHIP().to(dev)          # SD-2.1 VAE topology (83.65 M parameters), torch default init
    sched = ShiftSNRScheduler.from_scheduler(noise_scheduler=DDPMScheduler(), shift_mode="interpolated", shift_scale=6.0,
                                             scheduler_class=DDPMScheduler)
    pipe = MVDPipeline(model, sched, vae=vae)
    g = torch.Generator().manual_seed(7)
    embeds = torch.randn(1, 77, 1024, generator=g).to(dev)
    img = (torch.rand(1, 3, 8 * L_, 8 * L_, generator=g) * 2 - 1).to(dev)
    src, tgt = look_at(0.0)[None].to(dev), look_at(90.0)[None].to(dev)
    nsteps = args.e2e_steps

    def one_image():
        return pipe(prompt_embeds=embeds, height=8 * L_, width=8 * L_, num_inference_steps=nsteps, guidance_scale=1.0,
                    source_camera=src, target_camera=tgt, source_images=img, output_type="pt")["images"]

    def timed(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), out

    torch.manual_seed(OUTPUT_SEED)
    for _ in range(max(1, args.warmup)):
        out = one_image()
    assert torch.isfinite(out).all() and out.shape == (1, 3, 8 * L_, 8 * L_)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one_image()
    torch.cuda.synchronize()
    per_image = (time.perf_counter() - t0) / args.steps
    dumped = dump_outputs(args.dump_outputs, {"images": out}) if args.dump_outputs else None
    f_main, f_base = unet_flops(L_, L_, adapter=True), unet_flops(L_, L_)
    fl = nsteps * f_main + (1 if args.cached else nsteps) * f_base
    phases, shares, loop_tflops = None, None, None
    if args.full:
        t_enc, dist = timed(lambda: vae.encode(img).latent_dist.sample(), 5)
        lat = dist * vae.config.scaling_factor
        t_dec, _ = timed(lambda: vae.decode(lat / vae.config.scaling_factor).sample, 5)
        phases = {"vae_encode": round(t_enc * 1e3, 2), "vae_decode": round(t_dec * 1e3, 2),
                  "loop_and_glue": round((per_image - t_enc - t_dec) * 1e3, 2),
                  "per_denoising_step": round((per_image - t_enc - t_dec) / nsteps * 1e3, 3)}
        shares = {"vae": round((t_enc + t_dec) / per_image, 3), "loop": round(1 - (t_enc + t_dec) / per_image, 3)}
        loop_tflops = round(fl / max(per_image - t_enc - t_dec, 1e-9) / 1e12, 1)
    cpu = None if args.no_cpu_baseline or not args.full else cpu_baseline(1, 0, L_)
    line = {"metric": "images/sec end to end (VAE encode + denoising loop + VAE decode), 1 GPU", "value": round(1.0 / per_image, 4),
            "unit": "images/s", "seconds_per_image": round(per_image, 4), "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(per_image * 1e3, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic",
            "config": {"workload": f"e2e: one image as infer.py:111-122 runs it (B=1, guidance 1.0, camera + image conditioning, "
                                   f"{'cache_reference (Q5)' if args.cached else 'reference encoder re-run every step'})",
                       "image": f"{8 * L_}x{8 * L_}", "latent": f"{L_}x{L_}x4", "denoising_steps": nsteps, "text_tokens": 77,
                       "weights": "synthetic (UNet: seeded variance-preserving; VAE: torch default init), SD-2.1 shapes"},
            "phases_ms": phases, "shares": shares, "unet_tflops_in_loop": loop_tflops,
            "cpu_baseline": cpu, "kernel_src_sha": kernel_source_sha(), "full": bool(args.full), "outputs_dumped": dumped}
    print(json.dumps(line), flush=True)
    return 0


# Many-image shards (BASELINE configs[3] / [4]: 32 pairs per GPU) never read the batch-1 twins of the packed weights (the `.ws`
# convolution streams and the C > 640 LayerNorm-folded copies: launches with M <= 1024 rows, or <= 12 GFLOP up to M = 4608): they
# are packed lean, which is also what the start-up broadcast then moves (3.7 GB per rank instead of 6.5 GB).
LEAN_PACKING_FROM_PAIRS = 16


def launch_dry_run(args, D):
    """The N > 1 control flow of main() with the GPU work left out (CPU test of the self-launching entry): gloo process
    group from the launcher's environment, a weight-arena broadcast through the product's own helper, the barriers and the
    max-over-ranks reduction, rank 0's line.  The numbers mean nothing."""
    rank, world, _ = D.init_from_env("gloo", set_device=False)
    g = torch.Generator().manual_seed(7)
    ref = {"a.w": torch.randn(300, 64, generator=g).to(torch.bfloat16), "a.b": torch.randn(300, generator=g)}
    mine = ref if rank == 0 else {k: torch.zeros_like(v) for k, v in ref.items()}
    arenas, views = D.pack_into_arenas(mine)
    bc = D.broadcast_arenas(arenas.values(), 0)
    idents = D.gather_identities(int(os.environ.get("LOCAL_RANK", "0")))
    ok = all(torch.equal(views[k], ref[k]) for k in ref)
    D.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    D.barrier()
    elapsed = D.max_over_ranks(time.perf_counter() - t0, "cpu")
    if rank == 0:
        print(json.dumps({"metric": "launch dry run (no GPU work)", "value": 0.0, "unit": "forward-passes/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3, 3),
                          "weight_broadcast": {"bytes": bc["bytes"], "seconds": round(bc["seconds"], 4), "buckets": bc["buckets"],
                                               "backend": D.collective_library(), "rehearsal": True},
                          "ranks_seen": idents, "distinct_gpus": D.distinct_devices(idents),
                          "broadcast_ok": bool(ok), "dry_run": True}), flush=True)
    D.shutdown()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=list(WORKLOADS) + ["e2e"], default="cfg4")
    ap.add_argument("--e2e-steps", type=int, default=20, help="--workload e2e: denoising steps per image (infer.py's default)")
    ap.add_argument("--pairs", type=int, default=0, help="override pairs per GPU")
    ap.add_argument("--cached", action="store_true", help="reuse the step-invariant reference K/V (Q5) instead of re-running the encoder")
    ap.add_argument("--graph", action="store_true", help="replay each forward as one hipGraphLaunch (mvd_engine_set_graph); pays at batch 1 only")
    ap.add_argument("--global-ref-stats", action="store_true",
                    help="Q2 statistics over ALL ranks' batches (SURVEY 8e mode ii: one 323 KB all-gather per reference pass) instead of per replica")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-check", action="store_true", help="skip the determinism / cross-path output screens")
    ap.add_argument("--shapes-out", default="", help="write the per-shape kernel table of the profiled steps to this file")
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (64 = 512x512 images, 96 = the reference's 768x768 default, infer.py:187)")
    ap.add_argument("--attn-stats", choices=["flat", "peaked"], default="flat",
                    help="flat: variance-preserving query projections (near-uniform softmaxes, the default synthetic weights); peaked: every "
                         "to_q / to_q_ref scaled by --attn-q-scale so that a row's 8 largest probabilities hold > 90 %% of the mass, as in a "
                         "trained checkpoint -- the attention kernel's clock and rate depend on the operand statistics")
    ap.add_argument("--attn-q-scale", type=float, default=8.0, help="--attn-stats peaked: factor on the query projections")
    ap.add_argument("--encoder-weights", choices=["distinct", "frozen-copy"], default="distinct",
                    help="distinct (default, every round's line): the image encoder gets its own random weights -- two packed weight sets, "
                         "3.96 GB; frozen-copy: image_encoder.unet = a copy of base_unet, what the reference's default training config "
                         "produces (train_denoising_unet false: both are the frozen pretrained SD-2.1 UNet, training.py:60-65, "
                         "config/train_config.yaml:43) -- the engine then keeps ONE packed set for both passes (2.0 GB to broadcast)")
    ap.add_argument("--attn-nw", type=int, default=-1, help="measurement: force log2(waves per attention workgroup)")
    ap.add_argument("--debug-flags", type=int, default=0, help="measurement: mvd_debug_set_flags bits")
    ap.add_argument("--launch-dry-run", action="store_true",
                    help="control flow only (no GPU, gloo): process group, a small arena broadcast, barriers, max over ranks, rank 0's line")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the output screens, the per-kernel-class profile and roofline, the CPU "
                         "baseline, the attention-statistics proxy, e2e's per-phase times (each still off with its --no-* option)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32, rank 0's shard, "
                         "at most 64 MB: a larger output is a fixed seeded sample); inputs are seeded, the same on every run")
    args = ap.parse_args()
    if args.shapes_out and not args.full:
        ap.error("--shapes-out comes from the per-kernel-class profile: it needs --full")

    # ---- self-launch: `python bench.py --gpus N` without a launcher starts the N ranks itself.  Nothing in this process has
    # touched a GPU at this point (importing torch does not), and nothing will: the ranks are fresh children of
    # torch.distributed.run, whose stdout (rank 0's single JSON line) and exit code are passed through.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # the children's stdout is filtered: only a JSON line that carries "metric" is this program's stdout (communication
        # libraries chat on stdout -- "[Gloo] Rank 0 is connected to ..." in rehearsal mode); everything else goes to stderr
        proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
        for ln in proc.stdout:
            is_line = False
            if ln.lstrip().startswith("{"):
                try:
                    is_line = "metric" in json.loads(ln)
                except ValueError:
                    pass
            (sys.stdout if is_line else sys.stderr).write(ln)
            (sys.stdout if is_line else sys.stderr).flush()
        sys.exit(proc.wait())

    from mvd_amd import distributed as D
    if args.launch_dry_run:
        return launch_dry_run(args, D)
    # MVD_BENCH_REHEARSAL=1: every rank on cuda:0 with the gloo backend -- a one-GPU rehearsal of the N > 1 control flow
    # (weight broadcast, barriers, max over ranks); the numbers of such a run mean nothing
    rehearsal = os.environ.get("MVD_BENCH_REHEARSAL") == "1"
    # (init_from_env selects cuda:LOCAL_RANK before the RCCL process group is created)
    D.check_enough_devices(int(os.environ.get("WORLD_SIZE", "1")), rehearsal)     # before any process group exists
    rank, world, local = D.init_from_env("gloo" if rehearsal else "nccl")
    if rehearsal:
        local = 0
    if world != args.gpus:
        if rank == 0:
            print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using {world}", file=sys.stderr)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    if args.workload == "e2e":
        if world != 1:
            raise SystemExit("--workload e2e is a one-GPU workload")
        return e2e_workload(args, dev)
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    pairs, use_cam, use_img, desc = WORKLOADS[args.workload]
    if args.pairs:
        pairs = args.pairs

    # ---- model: rank 0 creates the synthetic weights, every rank packs buffers, one RCCL broadcast
    # (dedup_encoder_weights=False: the synthetic image-encoder weights differ from the base UNet's, as a trained checkpoint's
    #  do -- and the all-zero placeholders of ranks > 0 must not be "de-duplicated" into a different arena layout than rank 0's)
    model = MultiViewUNet(None, unet_config=UNetConfig.sd21(), init="empty", img_ref_scale=0.3,
                          cam_modulation_strength=0.2, cache_reference=args.cached,
                          dedup_encoder_weights="auto" if args.encoder_weights == "frozen-copy" else False,
                          small_batch_twins=pairs < LEAN_PACKING_FROM_PAIRS).to(dev)
    model.eval()
    model.use_hip_graph = args.graph
    if args.global_ref_stats:
        model.reference_stats_group = True
    q_scale = args.attn_q_scale if args.attn_stats == "peaked" else 1.0
    if rank == 0:
        fill_synthetic_weights(model, 0, q_scale)
        if args.encoder_weights == "frozen-copy" and model.image_encoder is not None:
            with torch.no_grad():
                base = dict(model.base_unet.named_parameters())
                for name, p in model.image_encoder.unet.named_parameters():
                    p.copy_(base[name])
            model.mark_weights_changed()
    else:
        with torch.no_grad():
            for p in model.parameters():
                p.zero_()
        model.mark_weights_changed()
    eng = model._sync_engine()
    bc = D.broadcast_engine_weights(eng, 0)
    # every rank's GPU, for rank 0's line (LOCAL_RANK as the launcher gave it: a rehearsal binds every rank to device 0)
    idents = D.gather_identities(int(os.environ.get("LOCAL_RANK", local)))
    weight_bytes = eng.weight_bytes()
    for p in model.parameters():           # fp32 masters are no longer needed on the device
        p.data = torch.empty(0, device=dev)
    model._dirty = False
    torch.cuda.empty_cache()

    if args.debug_flags:
        from mvd_amd import _lib as _L
        _L.lib().mvd_debug_set_flags(args.debug_flags)
    if args.attn_nw >= 0:
        from mvd_amd import _lib as _L
        _L.lib().mvd_debug_set_attention_nw(args.attn_nw)
    batch = make_batch(pairs, rank, dev, args.latent)
    kw = {}
    if use_cam:
        kw.update(source_camera=batch["src"], target_camera=batch["tgt"])
    if use_img:
        kw.update(source_image_latents=batch["lat"])

    def step():
        with torch.no_grad():
            return model(batch["sample"], batch["t"], batch["text"], **kw).sample

    out = None
    torch.manual_seed(OUTPUT_SEED)
    for _ in range(args.warmup):
        out = step()
    torch.cuda.synchronize()
    assert out is None or torch.isfinite(out).all(), "non-finite UNet output"
    check = None if args.no_check or not args.full else output_check(model, batch, kw, step, strict_cross=args.attn_stats == "flat")
    D.barrier()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        out = step()
    e1.record()
    torch.cuda.synchronize()
    D.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = D.max_over_ranks(elapsed, dev)
    gpu_ms = e0.elapsed_time(e1)
    # (before any further forward: the engine may hand back the same output buffer on the next call)
    dumped = dump_outputs(args.dump_outputs, {"sample": out}) if args.dump_outputs and rank == 0 else None

    forward_kind = "base" if not use_img else ("cached" if args.cached else "cold")
    f_base, f_main = unet_flops(args.latent, args.latent), unet_flops(args.latent, args.latent, adapter=True)
    if args.latent == 64:
        assert abs(f_base - F_BASE) < 1e7 and abs(f_main - F_ADAPTER_MAIN) < 1e7, (f_base, f_main)   # SURVEY 8d's figures
    flops_pair = f_base if not use_img else (f_main if args.cached else f_main + f_base)
    total_pairs = pairs * world
    value = total_pairs * args.steps / elapsed

    # ---- per-kernel-class timing with HIP events on the launch stream (rank 0, after the timed region)
    roofline = None
    classes = {}
    if args.full and not args.no_profile:
        nprof = min(args.steps, 3)
        eng.set_profiling(True)
        for _ in range(nprof):
            step()
        torch.cuda.synchronize()
        if args.shapes_out and rank == 0:
            with open(args.shapes_out, "w") as f:
                f.write(f"# {args.workload} {'cached' if args.cached else 'cold'} pairs={pairs}, {nprof} profiled steps, kernel_src_sha={kernel_source_sha()}\n")
                f.write(eng.profile_shapes())
        classes = eng.profile_summary()
        # the same launches measured INSIDE the forward's own schedule (encoder pass on the side stream): what a rocprofv3
        # --kernel-trace of the timed region averages, and what the overlapped step time is made of
        overl = {}
        if use_img and not args.cached and not args.graph and not (args.debug_flags & 16):
            eng.set_profiling(2)
            for _ in range(nprof):
                step()
            torch.cuda.synchronize()
            overl = eng.profile_summary()
        eng.set_profiling(False)
        tot_ms = sum(c["ms"] for c in classes.values())
        mf = {k: c for k, c in classes.items() if c["flops"] > 0}
        if mf:
            dom = max(mf, key=lambda k: mf[k]["ms"])
            c = mf[dom]
            ach = c["flops"] / (c["ms"] * 1e-3) / 1e12
            # HBM bytes per launch of that kernel class from the committed rocprofv3 --pmc passes of this command
            # (FETCH_SIZE x2 + WRITE_SIZE, gfx950 corrections; tools/pmc_summary.py) -- PMC cannot run inside bench.py
            traffic, traffic_file = None, None
            import glob
            for cand in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")), reverse=True):
                try:
                    pmc = json.load(open(cand))
                except (OSError, ValueError):
                    continue
                # only a summary taken on THIS kernel source state and THIS workload is quoted (else null)
                if (pmc.get("_meta", {}).get("kernel_src_sha") == kernel_source_sha() and args.workload == "cfg4" and args.latent == 64
                        and not args.cached and dom in pmc):
                    traffic, traffic_file = round(pmc[dom]["hbm_bytes_per_launch"]), os.path.relpath(cand, ROOT)
                    break
            roofline = {"bound": "mfma", "kernel": dom, "achieved": round(ach, 2), "peak": PEAK_BF16_MFMA / 1e12,
                        "unit": "TFLOP/s", "frac": round(ach * 1e12 / PEAK_BF16_MFMA, 4), "traffic": traffic,
                        "traffic_source": f"{traffic_file} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, same kernel sources)" if traffic else None,
                        "flops_per_launch": round(c["flops"] / c["launches"]),
                        "avg_launch_us": round(c["ms"] * 1e3 / c["launches"], 2),
                        "avg_launch_us_overlapped": round(overl[dom]["ms"] * 1e3 / overl[dom]["launches"], 2) if dom in overl else None,
                        "frac_overlapped": round(overl[dom]["flops"] / (overl[dom]["ms"] * 1e-3) / PEAK_BF16_MFMA, 4) if dom in overl else None,
                        "launches_per_step": c["launches"] // nprof,
                        "share_of_step_time": round(c["ms"] / tot_ms, 3),
                        "measured_over": f"{nprof} profiled steps after the timed region (HIP events on the launch stream): avg_launch_us / achieved / frac "
                                         "with the launches back to back on ONE stream, *_overlapped with the forward's own two-stream schedule",
                        "whole_forward_achieved": round(total_pairs * args.steps * flops_pair / elapsed / world / 1e12, 2),
                        "whole_forward_frac": round(total_pairs * args.steps * flops_pair / elapsed / world / PEAK_BF16_MFMA, 4)}
            for k in classes:
                classes[k] = {"launches": classes[k]["launches"] // nprof, "ms_per_step": round(classes[k]["ms"] / nprof, 3),
                              "tflops": round(classes[k]["flops"] / max(classes[k]["ms"], 1e-9) / 1e9, 1) if classes[k]["flops"] else None,
                              "gbps": round(classes[k]["bytes"] / max(classes[k]["ms"], 1e-9) / 1e6, 1) if classes[k]["bytes"] else None,
                              "ms_per_step_overlapped": round(overl[k]["ms"] / nprof, 3) if k in overl else None}

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(3, 1)

    if rank == 0:
        line = {
            "metric": "UNet forward-passes/sec @512x512 SD2.1+MV adapter", "value": round(value, 3),
            "unit": "forward-passes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"{args.workload}: {desc}", "pairs_per_gpu": pairs, "global_pairs": total_pairs,
                       "latent": f"{args.latent}x{args.latent}x4", "image": f"{8 * args.latent}x{8 * args.latent}", "text_tokens": 77, "forward": forward_kind, "hip_graph": bool(args.graph), "q2_statistics": "global" if args.global_ref_stats else "replica-local",
                       "gflop_per_pair": round(flops_pair / 1e9, 2), "parallelism": f"dp{world} (pairs sharded by object)",
                       "weights": "synthetic seeded, SD2.1 shapes (865.9M UNet x2 + 99.2M adapter + 19.1M camera)" if args.encoder_weights == "distinct"
                       else "synthetic seeded, SD2.1 shapes; image_encoder.unet = a frozen copy of base_unet (one packed weight set for both passes)",
                       "encoder_weights": args.encoder_weights, "encoder_weights_shared": bool(getattr(model, "encoder_weights_shared", False)),
                       "attn_stats": {"mode": args.attn_stats, **(softmax_stats_proxy(q_scale) if args.full else {"q_scale": q_scale})}},
            "roofline": roofline, "cpu_baseline": cpu, "output_check": check, "kernel_src_sha": kernel_source_sha(),
            "gpu_ms_per_step_events": round(gpu_ms / args.steps, 3),
            "weight_bytes_bf16_packed": weight_bytes,
            "weight_broadcast": {"bytes": bc["bytes"], "seconds": round(bc["seconds"], 4), "buckets": bc["buckets"],
                                 "backend": D.collective_library(), "rehearsal": rehearsal},
            "ranks_seen": idents, "distinct_gpus": D.distinct_devices(idents),
            "kernel_classes": classes, "full": bool(args.full), "outputs_dumped": dumped,
        }
        print(json.dumps(line), flush=True)
    D.shutdown()        # (after rank 0's line is out: a clean exit of every rank, no "process group not destroyed" noise)


if __name__ == "__main__":
    main()
