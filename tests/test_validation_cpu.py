"""Checkpoint scoring without a GPU: the fp64 restatements the GPU suite compares against (tests/losses_ref.py,
tests/ssim_ref.py) are pinned here -- on the reference's own ``compute_losses`` through tests/golden/g7_losses.npz, on
identities where the arithmetic is third-party (diffusers' add_noise / get_velocity, pytorch_msssim's SSIM) -- and the new
C entry points reject bad arguments on the host.

The fp32 drift test is the basis of the GPU suite's SSIM bounds (5e-6 natural, 2e-4 flat, 1e-6 identical): the SAME algorithm
evaluated in fp32 -- what pytorch_msssim itself computes in -- must sit inside a quarter of them.  Recorded on the seven inputs of
tests/ssim_ref.cases(): 6.1e-10 / 1.3e-8 / 5.3e-7 / 1.3e-8 on the four natural ones (the 512 x 512 figure is the fp32 mean over
252,004 map values, not the filter), 2.1e-7 on the flat 0.999 image and 3.2e-5 on constant 0.4 vs constant -0.7 at 11 x 11
(cancellation in ``filt(x^2) - mu^2`` against the small C2), 0 on identical images.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import losses_ref as LR
from tests import ssim_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g7(golden_dir):
    return np.load(os.path.join(golden_dir, "g7_losses.npz"))


@pytest.fixture(scope="module")
def lib():
    from mvd_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


G7_CASES = [(pt, name) for pt in ("epsilon", "v_prediction") for name in ("novae", "vae", "vae_ssim")]


def restate_g7(g7, pt, name):
    t = lambda k: torch.from_numpy(g7[k])          # noqa: E731
    return LR.compute_losses(t(f"{pt}_noise_pred"), t("noise"), t("noisy_latents"), t("timesteps"), t("target_latents"),
                             g7["alphas_cumprod"], g7["base_alphas_cumprod"], pt,
                             decode=LR.standin_decode if name != "novae" else None,
                             ssim_fn=(lambda x, y: SR.ssim(x, y, 2.0)) if name == "vae_ssim" else None)


@pytest.mark.parametrize("pt,name", G7_CASES)
def test_restatement_matches_the_reference_function(g7, pt, name):
    got = restate_g7(g7, pt, name)
    assert list(got) == [str(k) for k in g7["keys"]]
    for k, v in got.items():
        want = float(g7[f"{pt}_{name}_{k}"])
        print(pt, name, k, v, want)
        if want == 0.0:
            assert v == 0.0, k
        else:
            assert abs(v - want) <= 1e-5 * abs(want), (k, v, want)


def test_mirror_returns_the_recorded_keys(g7):
    from mvd_amd import validation as V
    assert list(V.LOSS_KEYS) == [str(k) for k in g7["keys"]] == list(LR.KEYS)
    assert V.SNR_GAMMA == LR.SNR_GAMMA == 5.0


def test_q10a_scalar_mse_times_mean_weight_is_not_the_weighted_mean(g7):
    """Q10(a): on the fixture the reference's value equals mean-MSE x mean-weight and differs from the per-sample weighted mean."""
    t = lambda k: torch.from_numpy(g7[k]).double()          # noqa: E731
    pred, noise = t("epsilon_noise_pred"), t("noise")
    b = t("base_alphas_cumprod")[torch.from_numpy(g7["timesteps"])]
    snr = b / (1 - b)
    w = torch.minimum(snr, torch.full_like(snr, 5.0)) / snr
    per_sample = ((pred - noise) ** 2).flatten(1).mean(1)
    want = float(g7["epsilon_novae_noise_loss"])
    assert abs(float(per_sample.mean() * w.mean()) - want) <= 1e-5 * want
    assert abs(float((per_sample * w).mean()) - want) > 1e-3 * want


def test_forward_diffusion_identities():
    g = torch.Generator().manual_seed(0)
    x0, eps = torch.randn(6, 4, 8, 8, generator=g).double(), torch.randn(6, 4, 8, 8, generator=g).double()
    acp = torch.cumprod(1 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2, 0)
    ts = torch.tensor([0, 3, 250, 500, 900, 999])
    a, s = (acp[ts] ** 0.5).view(-1, 1, 1, 1), ((1 - acp[ts]) ** 0.5).view(-1, 1, 1, 1)
    noisy, vel = LR.add_noise(x0, eps, ts, acp), LR.get_velocity(x0, eps, ts, acp)
    assert (a * noisy - s * vel - x0).abs().max() <= 1e-12
    assert (s * noisy + a * vel - eps).abs().max() <= 1e-12
    assert (LR.denoise(vel, noisy, ts, acp, "v_prediction") - x0).abs().max() <= 1e-12
    assert (LR.denoise(eps, noisy, ts, acp, "epsilon") - x0).abs().max() <= 1e-12 * float(1 / a.min())
    assert torch.equal(LR.denoise(x0, noisy, ts, acp, "sample"), x0)
    r = LR.noise_loss(vel, eps, x0, noisy, ts, acp, acp, "v_prediction")
    assert r["mse"] <= 1e-24 and r["latent_recon_loss"] <= 1e-24 and 0 < r["mean_snr_weight"] <= 1.0


def test_ssim_restatement_identities():
    a, b, R = 0.4, -0.7, 2.0
    c1 = (0.01 * R) ** 2
    x, y = torch.full((2, 3, 17, 23), a, dtype=torch.float64), torch.full((2, 3, 17, 23), b, dtype=torch.float64)
    assert abs(float(SR.ssim(x, y, R)) - (2 * a * b + c1) / (a * a + b * b + c1)) <= 1e-12
    assert abs(float(SR.gaussian_window().sum()) - 1.0) <= 1e-15
    g = torch.Generator().manual_seed(3)
    u, v = torch.rand(2, 3, 20, 31, generator=g), torch.rand(2, 3, 20, 31, generator=g)
    assert abs(float(SR.ssim(u, u, 1.0)) - 1.0) <= 1e-12
    assert abs(float(SR.ssim(u, v, 1.0)) - float(SR.ssim(v, u, 1.0))) <= 1e-15
    assert abs(float(SR.ssim_per_image(u, v, 1.0).mean()) - float(SR.ssim(u, v, 1.0))) <= 1e-15
    m = float(SR.mse(u, v))
    assert abs(SR.psnr(u, v, 2.0) - 10 * math.log10(4.0 / m)) <= 1e-12 and SR.psnr(u, u, 2.0) == math.inf


# the GPU suite's bounds (fixed by the feature's specification) over 4: the library's own precision must sit well inside them
DRIFT_BOUND = {"natural": 5e-6 / 4, "flat": 2e-4 / 4, "identical": 0.0}


def test_fp32_drift_of_the_ssim_algorithm_is_recorded():
    cases = SR.cases()
    assert len(cases) == 7
    for name, (x, y, R, kind) in cases.items():
        s64, s32 = float(SR.ssim(x, y, R)), float(SR.ssim(x, y, R, dtype=torch.float32))
        print(f"ssim fp32 drift {name}: fp64 {s64:.9f} fp32 {s32:.9f} |diff| {abs(s64 - s32):.3e}")
        assert abs(s64 - s32) <= DRIFT_BOUND[kind], (name, s64, s32)
        if kind == "identical":
            assert s64 == 1.0


# ------------------------------------------------------------------------------------------------ the C entry points, no GPU
def test_ws_bytes_functions_answer(lib):
    from mvd_amd import _lib as L
    assert lib.mvd_op_noise_loss_ws_bytes(32, 4 * 64 * 64) > 0
    assert lib.mvd_op_noise_loss_ws_bytes(1, 4) == 8
    assert lib.mvd_op_noise_loss_ws_bytes(3, 6) < 0 and "multiple of 4" in L.last_error()
    assert lib.mvd_op_noise_loss_ws_bytes(0, 4) < 0 and "batch" in L.last_error()
    with_ssim, without = lib.mvd_op_image_metrics_ws_bytes(32, 3, 512, 512, 1), lib.mvd_op_image_metrics_ws_bytes(32, 3, 512, 512, 0)
    assert with_ssim > without > 0
    assert lib.mvd_op_image_metrics_ws_bytes(1, 1, 11, 11, 1) == 8 + 16
    assert lib.mvd_op_image_metrics_ws_bytes(1, 3, 10, 64, 1) < 0 and "smaller than the 11-tap" in L.last_error()
    assert lib.mvd_op_image_metrics_ws_bytes(1, 3, 64, 10, 0) < 0 and "smaller than the 11-tap" in L.last_error()
    assert lib.mvd_op_image_metrics_ws_bytes(0, 3, 64, 64, 1) < 0 and "positive" in L.last_error()
    assert lib.mvd_op_image_metrics_ws_bytes(4096, 8, 256, 256, 1) < 0 and "2^31" in L.last_error()


def test_entry_points_reject_bad_arguments_on_the_host(lib):
    """Every failing call returns before any launch (the fake non-null pointers are never dereferenced on the host)."""
    from mvd_amd import _lib as L
    p = C.c_void_p(0x1000)
    assert lib.mvd_op_add_noise(None, p, p, p, p, 1000, p, None, 2, 8, None) == -1 and "null input" in L.last_error()
    assert lib.mvd_op_add_noise(p, p, p, p, p, 1000, None, None, 2, 8, None) == -1 and "neither" in L.last_error()
    assert lib.mvd_op_add_noise(p, p, p, p, p, 0, p, None, 2, 8, None) == -1 and "empty schedule" in L.last_error()
    assert lib.mvd_op_add_noise(p, p, p, p, p, 1000, p, None, 2, 6, None) == -1 and "multiple of 4" in L.last_error()
    assert lib.mvd_op_add_noise(p, p, p, p, p, 1000, p, None, 70000, 8, None) == -1 and "65535" in L.last_error()

    def nl(pred=p, noise=p, x0=p, noisy=p, ts=p, snr=p, T=1000, pt=1, den=None, res=p, batch=2, per=8, ws=p, wsb=1 << 20):
        return lib.mvd_op_noise_loss(pred, noise, x0, noisy, ts, p, p, snr, T, pt, 5.0, den, res, batch, per, ws, wsb, None)
    assert nl(pred=None) == -1 and "null input" in L.last_error()
    assert nl(snr=None) == -1 and "null input" in L.last_error()
    assert nl(pt=3) == -1 and "prediction_type 3" in L.last_error()
    assert nl(x0=None) == -1 and "need x0" in L.last_error()
    assert nl(pt=0, x0=None, den=p) == -1 and "denoised latents asked for" in L.last_error()
    assert nl(noisy=None, den=p) == -1 and "denoised latents asked for" in L.last_error()
    assert nl(per=10) == -1 and "multiple of 4" in L.last_error()
    assert nl(T=0) == -1 and "empty schedule" in L.last_error()
    assert nl(wsb=4) == -1 and "workspace of 4 bytes, need 16" in L.last_error()
    assert nl(ws=None) == -1 and "workspace" in L.last_error()

    def im(x=p, y=p, n=2, c=3, h=32, w=32, R=2.0, ssim=1, res=p, ws=p, wsb=1 << 20):
        return lib.mvd_op_image_metrics(x, y, n, c, h, w, R, ssim, res, None, ws, wsb, None)
    assert im(x=None) == -1 and "null input" in L.last_error()
    assert im(h=10) == -1 and "smaller than the 11-tap" in L.last_error()
    assert im(w=7, ssim=0) == -1 and "smaller than the 11-tap" in L.last_error()
    assert im(R=0.0) == -1 and "data_range" in L.last_error()
    assert im(c=0) == -1 and "positive" in L.last_error()
    assert im(wsb=8) == -1 and "workspace of 8 bytes" in L.last_error()
    assert im(n=1 << 20, c=8, h=64, w=64) == -1 and "2^31" in L.last_error()


def test_cpu_tensors_raise_everywhere():
    from mvd_amd import validation as V
    from mvd_amd._lib import MvdError
    from mvd_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    x = torch.zeros(2, 4, 8, 8)
    for cls in (DDPMScheduler, DDIMScheduler, DPMSolverMultistepScheduler):
        s = cls()
        with pytest.raises(MvdError, match="GPU only"):
            s.add_noise(x, x, torch.tensor([1, 2]))
        with pytest.raises(MvdError, match="GPU only"):
            s.get_velocity(x, x, [1, 2])
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(MvdError, match="GPU only"):
        V.SSIM(data_range=2.0)(img, img)
    with pytest.raises(MvdError, match="GPU only"):
        V.PeakSignalNoiseRatio(data_range=2.0)(img, img)
    with pytest.raises(MvdError, match="GPU only"):
        V.compute_losses(x, x, timesteps=[1, 2], scheduler=DDPMScheduler(), base_scheduler=DDPMScheduler())
    with pytest.raises(ValueError, match="default window"):
        V.SSIM(data_range=2.0, win_size=7)


def test_shim_reexports_compute_losses():
    sys.path.insert(0, os.path.join(ROOT, "integration"))
    try:
        for m in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[m]
        from src.training.losses import compute_losses
        from mvd_amd import validation as V
        assert compute_losses is V.compute_losses
    finally:
        sys.path.remove(os.path.join(ROOT, "integration"))
        for m in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[m]
