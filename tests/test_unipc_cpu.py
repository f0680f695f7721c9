"""UniPC (mvd_amd/scheduler.py ``UniPCMultistepScheduler``) on the host: the per-call coefficients of the fused
corrector + predictor kernel, pinned by the textbook restatement tests/unipc_ref.py and by first-principles identities instead of
diffusers (absent here); the stateful ``step`` / ``step_guided``; the ``sampler="unipc"`` switch of the factory and the launches
the loop issues; the C ABI.

* UniP order 2 (bh2, rhos_p = 0.5) without the corrector IS DPM-Solver++ 2M midpoint; UniP order 1 IS DPM-Solver++ order 1;
* on point-mass data the exact noise makes every order land on the point, corrector on;
* on Gaussian data the probability-flow ODE has a closed form: UniPC order 2 beats DPM-Solver++ 2M at 8 and 10 steps.
Trajectories here apply the host coefficients in fp64 torch, in the kernel's affine form."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mvd_amd import _lib as L
from mvd_amd.scheduler import DDPMScheduler, DPMSolverMultistepScheduler, ShiftSNRScheduler, UniPCMultistepScheduler
from tests import unipc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000


def _shifted(cls, **overrides):
    """The interpolated shift-6 schedule of SD-2.1's betas in ``cls``; ``overrides`` join the base config ``from_config`` reads."""
    base = DDPMScheduler()
    base.config = SimpleNamespace(**{**vars(base.config), **overrides})
    return ShiftSNRScheduler.from_scheduler(base, "interpolated", shift_scale=6.0, scheduler_class=cls)


def _apply(c, m, x, xl, h):
    """The kernel's map (mvd_op_unipc_step) in fp64: returns (y, xc, x0).  A term whose coefficient is 0 is skipped, as there."""
    x0 = c.a0 * m + c.a1 * x
    xc = x
    if c.corr:
        xc = c.cx * xl
        for k, v in zip((c.c0, c.c1, c.c2), h):
            if k != 0.0:
                xc = xc + k * v
        xc = xc + c.ct * x0
    y = c.px * xc + c.p0 * x0
    for k, v in zip((c.p1, c.p2), h):
        if k != 0.0:
            y = y + k * v
    return y, xc, x0


def _model(x, t):
    """an arbitrary smooth nonlinear 'network' of (x, t)"""
    return torch.tanh(1.3 * x + 0.001 * t) * (0.7 + t / 2000.0) + 0.2 * torch.sin(x * x)


def _unipc_run(s, x, model):
    """A whole UniPC trajectory from the host coefficients (call i, the orders a fresh run takes)."""
    nan = torch.full_like(x, float("nan"))
    xl, h = nan, [nan, nan, nan]
    for i, t in enumerate(s.timesteps.tolist()):
        x, xl, x0 = _apply(s.step_coefficients(i), model(x, t), x, xl, h)
        h = [x0] + h[:2]
    return x


def _dpm_run(s, x, model):
    d = None
    for i, t in enumerate(s.timesteps.tolist()):
        a0, a1, p, q, r, _ = s.step_coefficients(i)
        x0 = a0 * model(x, t) + a1 * x
        x = p * x + q * x0 + (r * d if r != 0.0 else 0.0)
        d = x0
    return x


@pytest.mark.parametrize("steps_offset", [0, 1])
@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_host_coefficients_match_the_numpy_restatement(order, solver_type, pred, spacing, steps_offset):
    acp = R.alphas_cumprod(_shifted(DDPMScheduler).betas)
    x0 = torch.randn(2, 4, 6, 6, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for disable in ((), (1, 3, 4)):
        s = _shifted(UniPCMultistepScheduler, solver_order=order, solver_type=solver_type, prediction_type=pred,
                     timestep_spacing=spacing, steps_offset=steps_offset, disable_corrector=disable)
        for n in (6, 9, 20):                                    # set_timesteps resets the state between runs
            s.set_timesteps(n)
            assert s.timesteps.tolist() == R.timesteps("dpm", T, n, spacing, steps_offset).tolist()
            assert s.sigmas.dtype == torch.float64 and len(s.sigmas) == n + 1 and float(s.sigmas[-1]) == 0.0
            ref = R.UniPC(acp, s.timesteps.tolist(), order, solver_type, pred, disable_corrector=disable)
            b, nan = x0.numpy().copy(), np.full(x0.shape, np.nan)
            for i, t in enumerate(s.timesteps.tolist()):
                c = s.step_coefficients(i)
                assert c.corr == (i > 0 and (i - 1) not in disable)     # the corrector runs exactly where diffusers' rule says
                # every call's map on the restatement's own state (sample, last sample, history), so that each of the n calls is
                # held to the bound on its own.  Two free-running fp64 trajectories of the epsilon model drift apart by the
                # trajectory's own sensitivity (measured 7.4e-9 at |x| = 73: order 2, bh1, epsilon, linspace, n = 20), which
                # says nothing about the coefficients; free-running runs are held to their identities in the tests below.
                m = _model(torch.from_numpy(b), t).numpy()
                h = (ref.outs[::-1] + [nan] * 3)[:3]
                xl = nan if ref.last_sample is None else ref.last_sample
                got, got_xc, got_x0 = _apply(c, m, b, xl, h)
                b = ref.step(m, b)
                assert np.isfinite(b).all()
                for g, w in ((got, b), (got_xc, ref.last_sample), (got_x0, ref.outs[-1])):
                    assert np.abs(g - w).max() <= 1e-10 * max(1.0, np.abs(w).max()), (disable, n, i)


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_unip_without_the_corrector_is_dpmsolver(spacing, pred):
    """UniP order 2 (bh2, rhos_p = 0.5) is DPM-Solver++ 2M midpoint, UniP order 1 is DPM-Solver++ order 1 (the DDIM step)."""
    x = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for order in (1, 2):
        for n in (6, 9, 20):
            uni = _shifted(UniPCMultistepScheduler, prediction_type=pred, timestep_spacing=spacing, solver_order=order,
                           solver_type="bh2", disable_corrector=range(n))
            dpm = _shifted(DPMSolverMultistepScheduler, prediction_type=pred, timestep_spacing=spacing, solver_order=order,
                           solver_type="midpoint")
            uni.set_timesteps(n)
            dpm.set_timesteps(n)
            assert uni.timesteps.tolist() == dpm.timesteps.tolist()
            assert not any(uni.step_coefficients(i).corr for i in range(n))
            a, b = _unipc_run(uni, x.clone(), _model), _dpm_run(dpm, x.clone(), _model)
            err = ((a - b).abs().max() / b.abs().max()).item()
            assert err <= 1e-12, (order, n, err)


def _point_mass_model(x0_star, acp, pred):
    def m(x, t):
        a = float(acp[t])
        eps = (x - math.sqrt(a) * x0_star) / math.sqrt(1 - a)
        return eps if pred == "epsilon" else math.sqrt(a) * eps - math.sqrt(1 - a) * x0_star
    return m


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_point_mass_is_exact(spacing, pred):
    g = torch.Generator().manual_seed(1)
    x0_star = torch.randn(2, 4, 4, 4, generator=g, dtype=torch.float64)
    xT = torch.randn(2, 4, 4, 4, generator=g, dtype=torch.float64)
    for n in (1, 2, 5, 20, 50):
        for order in (1, 2, 3):
            for st in ("bh1", "bh2"):
                s = _shifted(UniPCMultistepScheduler, prediction_type=pred, timestep_spacing=spacing, solver_order=order, solver_type=st)
                s.set_timesteps(n)
                assert all(s.step_coefficients(i).corr for i in range(1, n))
                x = _unipc_run(s, xT.clone(), _point_mass_model(x0_star, s.alphas_cumprod.double(), pred))
                assert (x - x0_star).abs().max().item() <= 1e-10, (n, order, st)


def _gaussian_errors(n, solver, spacing="linspace", mu=0.3, s=0.7):
    """max |sampler - exact| on N(mu, s^2) data, the set-up of tests/test_samplers_cpu.py::_gaussian_errors restated: the ideal
    denoiser D(x~, sigma) = mu + s^2/(s^2 + sigma^2) (x~ - mu) (x~ = x / alpha) is linear and the probability-flow ODE
    dx~/dsigma = (x~ - D)/sigma gives x~ - mu ~ sqrt(s^2 + sigma^2).  The reference is the exact ODE solution down to the last
    nonzero sigma, then one exact denoise (the last step onto the final sigma 0 returns the model's x0 there).  ``solver``: "2M"
    (DPM-Solver++ order 2, midpoint) or the UniPC order (bh2, corrector on)."""
    if solver == "2M":
        sch = _shifted(DPMSolverMultistepScheduler, timestep_spacing=spacing, solver_order=2, solver_type="midpoint")
    else:
        sch = _shifted(UniPCMultistepScheduler, timestep_spacing=spacing, solver_order=solver, solver_type="bh2")
    sch.set_timesteps(n)
    acp = sch.alphas_cumprod.double()
    ts = sch.timesteps.tolist()

    def model(x, t):                                    # the exact v of the Gaussian
        a = float(acp[t])
        x0 = mu + s * s / (s * s + (1 - a) / a) * (x / math.sqrt(a) - mu)
        eps = (x - math.sqrt(a) * x0) / math.sqrt(1 - a)
        return math.sqrt(a) * eps - math.sqrt(1 - a) * x0

    a0 = float(acp[ts[0]])
    xT = torch.randn(4096, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * math.sqrt(a0 * s * s + 1 - a0) \
        + math.sqrt(a0) * mu
    got = (_dpm_run if solver == "2M" else _unipc_run)(sch, xT.clone(), model)
    sig0, sig1 = sch._sig[0], sch._sig[-2]
    xt = mu + (xT / math.sqrt(a0) - mu) * math.sqrt((s * s + sig1 * sig1) / (s * s + sig0 * sig0))
    want = mu + s * s / (s * s + sig1 * sig1) * (xt - mu)
    return (got - want).abs().max().item()


@pytest.mark.parametrize("spacing", ["linspace", "trailing"])
def test_unipc_beats_dpmsolver_2m_at_few_steps_on_gaussian_data(spacing):
    """Measured (N(0.3, 0.7^2), interpolated shift-6 schedule, v_prediction, bh2, corrector on), max-abs error at
    n = 5 / 8 / 10 / 20 / 50:
      linspace   DPM-Solver++ 2M  8.79e-2  3.89e-2  1.58e-2  1.42e-2  9.15e-3
                 UniPC order 1    1.46e-1  1.32e-1  1.13e-1  5.54e-2  1.80e-2
                 UniPC order 2    6.10e-2  1.07e-2  6.17e-3  1.57e-2  5.83e-3
                 UniPC order 3    5.82e-2  2.29e-3  1.42e-2  1.49e-2  4.07e-3
      trailing   DPM-Solver++ 2M  8.87e-2  3.89e-2  1.56e-2  1.47e-2  9.59e-3
                 UniPC order 1    1.47e-1  1.33e-1  1.14e-1  5.60e-2  1.85e-2
                 UniPC order 2    6.15e-2  1.05e-2  6.55e-3  1.62e-2  6.18e-3
                 UniPC order 3    5.87e-2  1.93e-3  1.46e-2  1.52e-2  4.30e-3
    Asserted: UniPC order 2 below DPM-Solver++ 2M at n = 8 and 10 only.  At n = 20 it is the other way round (the last lambda jump
    dominates both), so nothing is asserted there."""
    ns = (5, 8, 10, 20, 50)
    e = {k: [_gaussian_errors(n, k, spacing) for n in ns] for k in ("2M", 1, 2, 3)}
    for k, v in e.items():
        print(spacing, k, " ".join(f"{x:.2e}" for x in v))
    for n in (8, 10):
        assert e[2][ns.index(n)] < e["2M"][ns.index(n)], (n, e)


def _fake_launch(calls):
    def launch(model_out, guidance_scale, c, sample, last, hist, xc_out, x0_out):
        if guidance_scale is not None:
            u, cc = model_out.chunk(2)
            model_out = u + guidance_scale * (cc - u)
        y, xc, x0 = _apply(c, model_out, sample, last, list(hist))
        calls.append((c, xc_out, x0_out))
        if xc_out is not None:
            xc_out.copy_(xc)
        if x0_out is not None:
            x0_out.copy_(x0)
        return y
    return launch


@pytest.mark.parametrize("order", [1, 2, 3])
def test_stateful_step_drives_the_same_trajectory(order):
    """``step`` / ``step_guided``'s own bookkeeping (step index from the first timestep, order ramp-up, ``lower_order_final``, the
    rotation of the history buffers, the last-sample buffer, their reset by set_timesteps) with the kernel replaced by its fp64 map
    on the host -- a test stand-in only.  The buffers start as NaN: reading a slot no step has written shows in the result."""
    acp = R.alphas_cumprod(_shifted(DDPMScheduler).betas)
    disable = (2,)
    s = _shifted(UniPCMultistepScheduler, solver_order=order, solver_type="bh1", timestep_spacing="trailing", disable_corrector=disable)
    calls = []
    s._launch_unipc = _fake_launch(calls)
    shape = (1, 4, 5, 5)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    nan = lambda: torch.full(shape, float("nan"), dtype=torch.float64)      # noqa: E731
    bufs = [nan() for _ in range(order)]
    s._bufs[(shape, torch.device("cpu"))] = (list(bufs), nan())
    for n in (12, 5):
        s.set_timesteps(n)
        assert s.step_index is None and s.lower_order_nums == 0 and s.this_order == 0
        a, b = x.clone(), x.numpy().copy()
        ref = R.UniPC(acp, s.timesteps.tolist(), order, "bh1", "v_prediction", disable_corrector=disable)
        for i, t in enumerate(s.timesteps.tolist()):
            mo = _model(a, t)
            a = s.step_guided(torch.cat([mo * 0.5, mo * 0.75]), 2.0, t, a).prev_sample if i % 2 else s.step(mo, t, a).prev_sample
            b = ref.step(_model(torch.from_numpy(b), t).numpy(), b)
            assert s.step_index == i + 1 and s.lower_order_nums == min(i + 1, order)
            assert s.this_order == min(order, i + 1, n - i)     # ramp-up at the start, lower_order_final at the end
        assert torch.isfinite(a).all()
        assert np.abs(a.numpy() - b).max() <= 1e-10 * max(1.0, np.abs(b).max()), n
        run = calls[-n:]
        assert [c.corr for c, _, _ in run] == [i > 0 and (i - 1) not in disable for i in range(n)]
        assert [c.p1 != 0.0 for c, _, _ in run] == [min(order, i + 1, n - i) >= 2 for i in range(n)]
        assert [c.p2 != 0.0 for c, _, _ in run] == [min(order, i + 1, n - i) >= 3 for i in range(n)]
        # the newest x0 goes into the oldest slot: the ``order`` buffers take turns, and no other tensor is ever allocated
        slots = [id(x0_out) for _, _, x0_out in run]
        assert set(slots) <= {id(t) for t in bufs} and all(slots[i] == slots[i - order] for i in range(order, n))
        assert len(set(slots[:order])) == min(order, n)
        # the last sample is stored exactly where the next call's corrector reads it
        assert [xc_out is not None for _, xc_out, _ in run] == [i + 1 < n and i not in disable for i in range(n)]
        with pytest.raises(ValueError, match="set_timesteps"):
            s.step(mo, 0, a)
    # a different shape in mid-trajectory is an error, not a silent first-order step
    s.set_timesteps(6)
    for t in s.timesteps.tolist()[:2]:
        x = s.step(_model(x, t), t, x).prev_sample
    other = torch.zeros(1, 4, 6, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="same shape"):
        s.step(other, s.timesteps.tolist()[2], other)


def test_lower_order_final_false_raises_at_the_last_step():
    s = _shifted(UniPCMultistepScheduler, solver_order=2, lower_order_final=False)
    s.set_timesteps(5)
    for i in range(4):
        s.step_coefficients(i)
    with pytest.raises(ValueError, match="zero final sigma"):
        s.step_coefficients(4)
    assert _shifted(UniPCMultistepScheduler, solver_order=1, lower_order_final=False).config.lower_order_final is False
    s1 = _shifted(UniPCMultistepScheduler, solver_order=1, lower_order_final=False)
    s1.set_timesteps(5)
    c = s1.step_coefficients(4)                             # order 1 onto sigma 0: y = x0 exactly
    assert (c.px, c.p0, c.p1, c.p2) == (0.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        s.step_coefficients(4, order=3)
    with pytest.raises(ValueError):
        s.step_coefficients(0, corrector=True)


@pytest.mark.parametrize("kw", [
    dict(predict_x0=False), dict(solver_p="anything"), dict(thresholding=True), dict(use_karras_sigmas=True),
    dict(use_exponential_sigmas=True), dict(use_beta_sigmas=True), dict(rescale_betas_zero_snr=True),
    dict(final_sigmas_type="sigma_min"), dict(solver_order=4), dict(solver_type="midpoint"), dict(prediction_type="sample"),
    dict(timestep_spacing="karras"),
])
def test_unsupported_options_raise(kw):
    with pytest.raises(ValueError):
        UniPCMultistepScheduler(**kw)


def test_set_timesteps_arguments_and_apg_x0_space():
    s = _shifted(UniPCMultistepScheduler)
    with pytest.raises(ValueError):
        s.step_coefficients(0)
    with pytest.raises(ValueError):
        s.set_timesteps(4, timesteps=[900, 600])
    with pytest.raises(ValueError):
        s.set_timesteps(timesteps=[1000, 10])
    s.set_timesteps(timesteps=[900, 600, 300])
    assert s.timesteps.tolist() == [900, 600, 300] and s.num_inference_steps == 3
    assert type(UniPCMultistepScheduler.from_config(DDPMScheduler().config)) is UniPCMultistepScheduler
    assert s.order == 1 and s.init_noise_sigma == 1.0
    z = torch.zeros(2, 4, 4, 4)
    with pytest.raises(ValueError, match="UniPC"):
        s.step_guided(torch.cat([z, z]), 3.0, 900, z, apg=dict(eta=0.5, space="x0"))


# ------------------------------------------------------------------------------------------------ factory, loop, val
TINY = dict(dtype=torch.float32, cam_output_dim=96, cam_hidden_dim=48, init="empty")


def test_factory_offers_unipc():
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import create_mvd_pipeline
    from mvd_amd.pipeline import SAMPLERS
    assert SAMPLERS == ("ddpm", "ddim", "dpmsolver++", "unipc")
    ref = create_mvd_pipeline(None, unet_config=UNetConfig.tiny(), **TINY).scheduler
    assert type(ref) is DDPMScheduler                              # the default is unchanged
    s = create_mvd_pipeline(None, sampler="unipc", unet_config=UNetConfig.tiny(), **TINY).scheduler
    assert type(s) is UniPCMultistepScheduler and torch.equal(s.alphas_cumprod, ref.alphas_cumprod)
    assert s.config.solver_order == 2 and s.config.solver_type == "bh2" and s.config.prediction_type == "v_prediction"
    with pytest.raises(ValueError, match="sampler"):
        create_mvd_pipeline(None, sampler="euler", unet_config=UNetConfig.tiny(), **TINY)


def test_snapshot_config_reaches_unipc(tmp_path):
    import json
    from mvd_amd.pipeline import _make_scheduler
    os.makedirs(tmp_path / "scheduler")
    json.dump({"_class_name": "DDIMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012,
               "beta_schedule": "scaled_linear", "prediction_type": "epsilon", "steps_offset": 1, "clip_sample": False,
               "set_alpha_to_one": False, "timestep_spacing": "trailing"},
              open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    s = _make_scheduler(str(tmp_path), "unipc")
    assert type(s) is UniPCMultistepScheduler
    assert s.config.timestep_spacing == "trailing" and s.config.steps_offset == 1 and s.config.prediction_type == "epsilon"
    assert torch.equal(s.alphas_cumprod, _make_scheduler(str(tmp_path), "ddpm").alphas_cumprod)


class _StubUNet:
    deepcache = None

    def _exec_device(self):
        return torch.device("cpu")

    def __call__(self, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None, **kw):
        return SimpleNamespace(sample=torch.tanh(sample) * 0.5 + 0.01 * encoder_hidden_states.mean())


@pytest.mark.parametrize("rescale", [0.0, 0.7])
def test_loop_issues_one_launch_per_step_and_two_with_rescale(monkeypatch, rescale):
    """A stub UNet under the real loop and the real scheduler, the ``ops`` entries replaced by host stand-ins that count: plain
    guidance is exactly one ``unipc_step`` per step (guided), rescale is ``cfg_rescale`` + one unguided ``unipc_step``."""
    from mvd_amd import ops
    from mvd_amd.pipeline import MVDDenoiser
    count = {"unipc_step": [], "cfg_rescale": 0}

    def unipc_step(model_out, sample, a0, a1, px, p0, p1=0.0, p2=0.0, corr=False, cx=0.0, c0=0.0, c1=0.0, c2=0.0, ct=0.0,
                   last_sample=None, h0=None, h1=None, h2=None, guidance_scale=None, out=None, xc_out=None, x0_out=None):
        from mvd_amd.scheduler import UniPCCoefficients
        count["unipc_step"].append(guidance_scale)
        if guidance_scale is not None:
            u, c = model_out.chunk(2)
            model_out = u + guidance_scale * (c - u)
        y, xc, x0 = _apply(UniPCCoefficients(a0, a1, corr, cx, c0, c1, c2, ct, px, p0, p1, p2), model_out, sample, last_sample,
                           [h0, h1, h2])
        if xc_out is not None:
            xc_out.copy_(xc)
        if x0_out is not None:
            x0_out.copy_(x0)
        return y

    def cfg_rescale(uncond_cond, guidance_scale, guidance_rescale, out=None):
        count["cfg_rescale"] += 1
        u, c = uncond_cond.chunk(2)
        return u + guidance_scale * (c - u)             # (the statistics are the GPU tests' business)

    def forbidden(*a, **k):
        raise AssertionError("the UniPC loop issued a launch of another sampler")

    monkeypatch.setattr(ops, "unipc_step", unipc_step)
    monkeypatch.setattr(ops, "cfg_rescale", cfg_rescale)
    for name in ("cfg_combine", "sampler_step", "sampler_step_rescaled", "sampler_step_apg", "apg", "ddpm_step"):
        monkeypatch.setattr(ops, name, forbidden)
    sched = _shifted(UniPCMultistepScheduler)
    g = torch.Generator().manual_seed(6)
    steps = 7
    out = MVDDenoiser(_StubUNet(), sched)(torch.randn(2, 3, 8, generator=g), steps, 3.0,
                                          negative_prompt_embeds=torch.randn(2, 3, 8, generator=g),
                                          latents=torch.randn(2, 4, 8, 8, generator=g), guidance_rescale=rescale)
    assert torch.isfinite(out).all() and out.shape == (2, 4, 8, 8)
    assert len(count["unipc_step"]) == steps
    if rescale:
        assert count["cfg_rescale"] == steps and all(gs is None for gs in count["unipc_step"])
    else:
        assert count["cfg_rescale"] == 0 and all(gs == 3.0 for gs in count["unipc_step"])


def test_val_hands_the_sampler_key_to_the_factory(monkeypatch, tmp_path):
    """``mvd_amd.val``'s ``sampler`` config key reaches ``create_mvd_pipeline`` as it is."""
    import mvd_amd.mvd_unet as U
    from mvd_amd import val as V
    seen = {}

    class Stop(Exception):
        pass

    def fake_create(**kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(U, "create_mvd_pipeline", fake_create)
    ckpt = tmp_path / "c.ckpt"
    ckpt.write_bytes(b"")
    config = dict(architecture="x", torch_dtype="float32", use_camera_conditioning=True, use_image_conditioning=True,
                  img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96, cam_hidden_dim=48, simple_encoder=False,
                  sampler="unipc")
    with pytest.raises(Stop):
        V.setup_pipeline(config, str(ckpt), "cpu")
    assert seen["sampler"] == "unipc"


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_sigs_and_library_agree_on_the_entry_point():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    m = re.search(r"\bint\s+mvd_op_unipc_step\s*\(([^)]*)\)\s*;", hdr)
    assert m, "mvd_op_unipc_step is not declared in include/mvd_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    want = [C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int if p.startswith("int ") else C.c_float
            for p in params]
    assert all(p.startswith(("const float*", "float*", "void*", "int64_t ", "int ", "float ")) for p in params), params
    restype, argtypes = L._SIGS["mvd_op_unipc_step"]
    assert restype is C.c_int and argtypes == want
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "model_out", "guided", "guidance_scale", "sample", "last_sample", "h0", "h1", "h2", "a0", "a1", "corr", "cx", "c0", "c1",
        "c2", "ct", "px", "p0", "p1", "p2", "out", "xc_out", "x0_out", "n", "stream"]
    lib = L.lib()
    assert "mvd_op_unipc_step" in L.EXPORTED_SYMBOLS and hasattr(lib, "mvd_op_unipc_step")
    # the argument checks run on the host, before any launch
    assert lib.mvd_op_unipc_step(None, 0, 0.0, None, None, None, None, None, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, None, None, None, 8,
                                 None) == -1
    assert "unipc_step" in L.last_error()
    src = open(os.path.join(ROOT, "mvd_amd", "_build.py")).read()
    assert '"apg.hip", "unipc.hip"' in src
