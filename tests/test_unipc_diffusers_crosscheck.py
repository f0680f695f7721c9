"""Cross-check of tests/unipc_ref.py and ``mvd_amd.scheduler.UniPCMultistepScheduler`` against diffusers' own
``UniPCMultistepScheduler`` -- runs only where diffusers is installed (it is not in the image the suite is built for, where this
module skips like tests/test_diffusers_crosscheck.py).  diffusers keeps its sigmas in fp32 and runs the solves in the sample's
dtype, so the comparison is in fp64 samples to 1e-5 relative: the sigmas' rounding, not the algebra."""
import numpy as np
import pytest
import torch

diffusers = pytest.importorskip("diffusers", reason="diffusers is not installed in this image (UniPC stays pinned by tests/unipc_ref.py)")

from mvd_amd.scheduler import DDPMScheduler, ShiftSNRScheduler, UniPCMultistepScheduler  # noqa: E402
from tests import unipc_ref as R  # noqa: E402


def _model(x, t):
    return torch.tanh(1.3 * x + 0.001 * t) * (0.7 + t / 2000.0) + 0.2 * torch.sin(x * x)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
def test_restatement_follows_diffusers(order, solver_type, spacing):
    ours = ShiftSNRScheduler.from_scheduler(DDPMScheduler(), "interpolated", shift_scale=6.0, scheduler_class=UniPCMultistepScheduler)
    theirs = diffusers.UniPCMultistepScheduler(trained_betas=ours.betas.numpy(), solver_order=order, solver_type=solver_type,
                                               prediction_type="v_prediction", timestep_spacing=spacing, final_sigmas_type="zero")
    acp = R.alphas_cumprod(ours.betas)
    x0 = torch.randn(2, 4, 6, 6, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for n in (6, 9, 20):
        theirs.set_timesteps(n)
        ts = theirs.timesteps.tolist()
        assert ts == R.timesteps("dpm", 1000, n, spacing, 0).tolist()
        ref = R.UniPC(acp, ts, order, solver_type, "v_prediction")
        a, b = x0.clone(), x0.numpy().copy()
        for t in ts:
            a = theirs.step(_model(a, t), t, a).prev_sample
            b = ref.step(_model(torch.from_numpy(b), t).numpy(), b)
        assert np.abs(a.numpy() - b).max() <= 1e-5 * max(1.0, np.abs(b).max()), n
