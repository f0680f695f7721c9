#!/usr/bin/env python3
"""A guided DPM-Solver++ 2M loop on the tiny topology, for a kernel trace of the loop's own launches: with a scheduler that has
``step_guided`` every step is ONE ``sampler_step_kernel`` launch and no ``cfg_combine_kernel``.

    rocprofv3 --kernel-trace --stats -d OUT -o sampler -- python tools/probe_sampler_loop.py [steps=20] [guidance=3.0]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mvd_amd.pipeline import MVDDenoiser
from mvd_amd.scheduler import DDPMScheduler, DPMSolverMultistepScheduler, ShiftSNRScheduler
from tests.parity_util import build_pair, make_inputs

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
gs = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
cfg, params, model = build_pair("tiny", 0, 96, 48)
inp = make_inputs(cfg, 2, 16, 7, seed=31, cam_dim=96)
sched = ShiftSNRScheduler.from_scheduler(DDPMScheduler(), "interpolated", shift_scale=6.0,
                                         scheduler_class=DPMSolverMultistepScheduler)
neg = torch.randn(2, 7, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(5))
model.fourier_projection = inp["proj"]
out = MVDDenoiser(model, sched)(inp["text"].cuda(), steps, gs, negative_prompt_embeds=neg.cuda(), latents=inp["sample"].cuda(),
                                source_camera=inp["src"].cuda(), target_camera=inp["tgt"].cuda(),
                                source_image_latents=inp["lat"].cuda())
torch.cuda.synchronize()
assert torch.isfinite(out).all()
print(f"dpmsolver++ 2M, {steps} steps, guidance {gs}: ok, |latents| max {out.abs().max().item():.3f}")
