"""Drop-in for the forward-only part of the reference's src/training/losses.py (imported by src/training/training.py:19 and
val.py): ``compute_losses`` with the reference's signature and keys, on the GPU.  ``PerceptualLoss`` (a pretrained VGG-16) is
not provided: pass any callable as ``perceptual_loss_fn``.  ``SSIM`` / ``PeakSignalNoiseRatio`` stand in for pytorch_msssim's and
torchmetrics' classes of the same name (val.py:69-75)."""
from mvd_amd.validation import compute_losses  # noqa: F401
from mvd_amd.validation import SSIM, PeakSignalNoiseRatio, ValidationScorer  # noqa: F401
