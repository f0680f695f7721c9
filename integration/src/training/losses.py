"""Drop-in for the forward-only part of the reference's src/training/losses.py (imported by src/training/training.py:19 and
val.py): ``compute_losses`` with the reference's signature and keys, on the GPU.  ``PerceptualLoss`` is the reference's class on
this project's VGG-16 kernels (mvd_amd/perceptual.py: the same constructor, ``__call__`` and ``.to``; the weights come from the
local torch hub cache or a path, nothing is downloaded); ``compute_losses`` takes it -- or any other callable -- as
``perceptual_loss_fn``.  ``SSIM`` / ``PeakSignalNoiseRatio`` stand in for pytorch_msssim's and torchmetrics' classes of the same
name (val.py:69-75)."""
from mvd_amd.perceptual import PerceptualLoss  # noqa: F401
from mvd_amd.validation import compute_losses  # noqa: F401
from mvd_amd.validation import SSIM, PeakSignalNoiseRatio, ValidationScorer  # noqa: F401
