#!/usr/bin/env python3
"""Regenerate tests/golden/g7_losses.npz from the reference's own ``compute_losses`` (src/training/losses.py) and
``compute_snr`` (src/training/scheduler.py):

    MVD_REFERENCE=/path/to/reference python tests/golden/make_golden_losses.py

The reference module imports ``icecream`` (a debug printer) and ``torchvision`` (``models`` / ``transforms``, used only by its
VGG perceptual loss, which this fixture never builds); neither is needed for the arithmetic, so no-op stand-ins go into
``sys.modules`` first, as make_golden.py does for icecream.  Nothing of the reference is copied: the file holds the seeded
inputs and what the reference RETURNED for them.

Inputs: (6, 4, 8, 8) tensors, timesteps [0, 3, 250, 500, 900, 999], prediction types epsilon and v_prediction, each without a
VAE, with the stand-in VAE (tests/losses_ref.standin_decode: parameter-free and smooth), and with the stand-in VAE plus an
SSIM callable (tests/ssim_ref.ssim at data_range 2: pytorch_msssim is not installed, so the fixture pins what the function
DOES with the callable's value, not the SSIM arithmetic, which tests/ssim_ref.py restates from its definition).
``scheduler`` and ``base_scheduler`` are two DIFFERENT schedules (SD-2.1's scaled-linear betas with the SNR divided by 6, and
the unshifted one) so that which object feeds which formula is pinned (Q10b).  The scheduler stand-in carries
``config.prediction_type``, ``alphas_cumprod`` and diffusers' ``get_velocity`` formula -- third-party arithmetic that the
fixture does not pin (tests/test_validation_cpu.py pins it by identities).
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/: losses_ref, ssim_ref
REF = os.environ.get("MVD_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src", "training")):
    sys.exit("set MVD_REFERENCE to a checkout of the reference project (it has src/training/losses.py)")
sys.path.insert(0, REF)

_ic = types.ModuleType("icecream")
_ic.ic = lambda *a, **k: None
sys.modules.setdefault("icecream", _ic)
if "torchvision" not in sys.modules:
    _tv, _m, _t = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.transforms")
    _m.VGG16_Weights = _m.vgg16 = _t.Normalize = None
    _tv.models, _tv.transforms = _m, _t
    sys.modules.update({"torchvision": _tv, "torchvision.models": _m, "torchvision.transforms": _t})

import losses_ref as LR  # noqa: E402
import ssim_ref as SR  # noqa: E402
from src.training.losses import compute_losses  # noqa: E402

TIMESTEPS = [0, 3, 250, 500, 900, 999]
CASES = (("novae", False, False), ("vae", True, False), ("vae_ssim", True, True))


class StandinScheduler:
    def __init__(self, alphas_cumprod, prediction_type):
        self.alphas_cumprod = alphas_cumprod
        self.config = SimpleNamespace(prediction_type=prediction_type, num_train_timesteps=len(alphas_cumprod))

    def get_velocity(self, sample, noise, timesteps):            # diffusers-0.32.2 DDPMScheduler.get_velocity
        acp = self.alphas_cumprod.to(dtype=sample.dtype)[timesteps]
        a, s = (acp ** 0.5).flatten(), ((1 - acp) ** 0.5).flatten()
        while a.dim() < sample.dim():
            a, s = a.unsqueeze(-1), s.unsqueeze(-1)
        return a * noise - s * sample


class StandinVAE:
    config = SimpleNamespace(scaling_factor=LR.STANDIN_SCALING_FACTOR)

    def decode(self, z):
        return SimpleNamespace(sample=LR.standin_decode(z))


def schedules():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    base = torch.cumprod(1.0 - betas, dim=0)
    snr = base / (1.0 - base) / 6.0
    return snr / (1.0 + snr), base


def main():
    g = torch.Generator().manual_seed(7)
    acp, base_acp = schedules()
    ts = torch.tensor(TIMESTEPS)
    x0 = 0.18215 * 4.0 * torch.randn(6, 4, 8, 8, generator=g)
    noise = torch.randn(6, 4, 8, 8, generator=g)
    a, s = (acp[ts] ** 0.5).view(-1, 1, 1, 1), ((1 - acp[ts]) ** 0.5).view(-1, 1, 1, 1)
    noisy = a * x0 + s * noise
    out = dict(timesteps=ts.numpy(), alphas_cumprod=acp.numpy(), base_alphas_cumprod=base_acp.numpy(), target_latents=x0.numpy(),
               noise=noise.numpy(), noisy_latents=noisy.numpy())
    keys = None
    for pt in ("epsilon", "v_prediction"):
        truth = noise if pt == "epsilon" else a * noise - s * x0
        pred = truth + 0.3 * torch.randn(6, 4, 8, 8, generator=g)          # an imperfect prediction
        out[f"{pt}_noise_pred"] = pred.numpy()
        sched, base = StandinScheduler(acp, pt), StandinScheduler(base_acp, pt)
        for name, with_vae, with_ssim in CASES:
            r = compute_losses(pred, noise, noisy_latents=noisy, timesteps=ts, target_latents=x0,
                               vae=StandinVAE() if with_vae else None, scheduler=sched, base_scheduler=base,
                               ssim_loss_fn=(lambda x, y: SR.ssim(x, y, 2.0).float()) if with_ssim else None)
            assert keys in (None, list(r)), (keys, list(r))
            keys = list(r)
            for k, v in r.items():
                out[f"{pt}_{name}_{k}"] = np.asarray(float(v), dtype=np.float64)
    out["keys"] = np.array(keys)
    path = os.path.join(HERE, "g7_losses.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
