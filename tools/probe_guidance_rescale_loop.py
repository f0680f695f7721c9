#!/usr/bin/env python3
"""A guided loop with guidance rescale on the tiny topology, for a kernel trace of the loop's own launches: every step is ONE
``sampler_step_rescaled_kernel`` launch, and neither ``cfg_combine_kernel`` nor ``sampler_step_kernel`` runs -- with any of the three
samplers (DDPM's step is the same affine form).

    rocprofv3 --kernel-trace --stats -d OUT -o rescale -- python tools/probe_guidance_rescale_loop.py [sampler=dpmsolver++] [steps=20]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mvd_amd.pipeline import MVDDenoiser, _make_scheduler
from tests.parity_util import build_pair, make_inputs

sampler = sys.argv[1] if len(sys.argv) > 1 else "dpmsolver++"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
gs, phi = 3.0, 0.7
cfg, params, model = build_pair("tiny", 0, 96, 48)
inp = make_inputs(cfg, 2, 16, 7, seed=31, cam_dim=96)
sched = _make_scheduler(None, sampler)
neg = torch.randn(2, 7, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(5))
model.fourier_projection = inp["proj"]
out = MVDDenoiser(model, sched)(inp["text"].cuda(), steps, gs, negative_prompt_embeds=neg.cuda(), latents=inp["sample"].cuda(),
                                source_camera=inp["src"].cuda(), target_camera=inp["tgt"].cuda(),
                                source_image_latents=inp["lat"].cuda(), guidance_rescale=phi)
torch.cuda.synchronize()
assert torch.isfinite(out).all()
print(f"{sampler}, {steps} steps, guidance {gs}, guidance_rescale {phi}: ok, |latents| max {out.abs().max().item():.3f}")
