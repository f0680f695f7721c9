"""Drop-in for /root/reference/src/training/scheduler.py (imported by mvd_unet.py:9).  The DDIM / DPM-Solver++ classes are
extras of this project (the reference has none): they take the place of diffusers' classes of the same name."""
from mvd_amd.scheduler import DDPMScheduler, ShiftSNRScheduler, SNR_to_betas, compute_snr  # noqa: F401
from mvd_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: F401
