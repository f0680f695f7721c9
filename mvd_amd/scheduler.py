"""Host-side scheduler math for the denoising loop.

* ``compute_snr`` / ``SNR_to_betas`` / ``ShiftSNRScheduler`` mirror /root/reference/src/training/scheduler.py:16-150
  (pinned by tests/golden/g4_shift_snr.npz, captured from the reference's own functions).
* ``DDPMScheduler`` restates the part of diffusers-0.32.2 ``DDPMScheduler`` the reference uses
  (``from_config(..., trained_betas=)``, ``set_timesteps``, ``step`` with ``variance_type="fixed_small"``,
  epsilon / v_prediction, no sample clipping -- the SD-2.1 scheduler config).  diffusers is not installed here, so
  this part is unpinned (checked against a numpy restatement in oracle/scheduler.py only).
* ``DDIMScheduler`` (Song et al. 2021) and ``DPMSolverMultistepScheduler`` (Lu et al. 2022, DPM-Solver++ multistep,
  data prediction, orders 1 / 2) restate the diffusers-0.32.2 algebra of those classes for the config subset named in
  their docstrings; anything outside it raises ValueError.  Also unpinned against diffusers; pinned instead by
  first-principles identities (tests/test_samplers_cpu.py: DDIM(eta=1) == the DDPM step, DDIM(eta=0) == DPM-Solver++
  order 1, exactness on point-mass data, convergence to the exact probability-flow ODE solution on Gaussian data).

Everything here is scalar / length-1000 vector math on the host; the per-step tensor update is one fused HIP
kernel (``mvd_op_ddpm_step``, ``mvd_op_sampler_step``) whose coefficients are computed here, so the loop never syncs
the device.

* Guidance rescale (Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4) restates
  diffusers-0.32.2 ``rescale_noise_cfg``: per batch row, m' = phi * m * std(cond) / std(m) + (1 - phi) * m with torch's unbiased
  std over the row and no epsilon (std(m) == 0 gives what IEEE arithmetic gives).  It is applied to the guided model output
  whatever the prediction type, only when guidance is active (``guidance_scale > 1``) and ``guidance_rescale > 0``; the
  statistics, the rescale and the step are ONE launch (``mvd_op_sampler_step_rescaled``).  Also unpinned against diffusers;
  pinned by the fp64 restatement in tests/guidance_ref.py and its identities (tests/test_guidance_rescale_cpu.py).
* Adaptive projected guidance (Sadat, Hilliges and Weber, ICLR 2025, "Eliminating Oversaturation and Artifacts of High Guidance
  Scales in Diffusion Models") restates diffusers' ``normalized_guidance`` with ``use_original_formulation=True``: ``APG`` holds
  the setting, the update itself is in the docstring of ``ops.apg``.  Applied only when guidance is active; the projection, the
  norm cap, the momentum update, the optional rescale and the step are ONE launch (``mvd_op_sampler_step_apg``).  The schedulers
  hold no APG state: the momentum buffer is the caller's.  Unpinned against diffusers; pinned by tests/apg_ref.py.
* ``UniPCMultistepScheduler`` (Zhao et al., NeurIPS 2023) restates diffusers-0.32.2's class of that name for
  data prediction, orders 1 - 3, bh1 / bh2: the corrector of the previous step and the predictor of this one are ONE launch
  (``mvd_op_unipc_step``).  Unpinned against diffusers; pinned by tests/unipc_ref.py and the identity UniP-2 (bh2) == DPM-Solver++ 2M.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Any, NamedTuple, Optional

import numpy as np
import torch


class APG:
    """The setting of adaptive projected guidance: ``eta`` in [0, 1] scales the part of the guidance update parallel to the
    conditional prediction (1: plain guidance, 0: the orthogonal part alone), ``norm_threshold`` >= 0 caps the update's norm per
    batch row (0: no cap), ``momentum`` in (-1, 1) is the running average's coefficient over the steps (the paper uses negative
    values; 0: none), ``space`` is "output" (the projection on the raw model output, as diffusers applies it) or "x0" (on the
    denoised prediction, the paper's setting).  ``APG.of(value)`` also takes a dict of these keys, a tuple / list in this order,
    or ``"eta,norm_threshold,momentum[,space]"``; ``None`` stays ``None``."""

    SPACES = ("output", "x0")
    __slots__ = ("eta", "norm_threshold", "momentum", "space")

    def __init__(self, eta: float = 0.0, norm_threshold: float = 0.0, momentum: float = 0.0, space: str = "output"):
        try:
            eta, norm_threshold, momentum = float(eta), float(norm_threshold), float(momentum)
        except (TypeError, ValueError):
            raise ValueError(f"apg: eta, norm_threshold and momentum must be numbers, got {(eta, norm_threshold, momentum)!r}") from None
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"apg: eta={eta!r} must lie in [0, 1]")
        if not 0.0 <= norm_threshold < math.inf:
            raise ValueError(f"apg: norm_threshold={norm_threshold!r} must be finite and >= 0 (0: off)")
        if not -1.0 < momentum < 1.0:
            raise ValueError(f"apg: momentum={momentum!r} must lie in (-1, 1)")
        if space not in self.SPACES:
            raise ValueError(f"apg: space={space!r}: expected one of {self.SPACES}")
        object.__setattr__(self, "eta", eta)
        object.__setattr__(self, "norm_threshold", norm_threshold)
        object.__setattr__(self, "momentum", momentum)
        object.__setattr__(self, "space", space)

    def __setattr__(self, name, value):
        raise AttributeError("APG is immutable")

    @classmethod
    def of(cls, value) -> "Optional[APG]":
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            unknown = set(value) - set(cls.__slots__)
            if unknown:
                raise ValueError(f"apg: unknown keys {sorted(unknown)} (expected {cls.__slots__})")
            return cls(**value)
        if isinstance(value, str):
            value = [v.strip() for v in value.split(",")]
        if isinstance(value, (tuple, list)) and 1 <= len(value) <= 4:
            return cls(*value)
        raise ValueError(f"apg: expected APG, a dict, or eta,norm_threshold,momentum[,space], got {value!r}")

    def kwargs(self):
        """the keywords of ``ops.apg`` / ``ops.sampler_step_apg`` (without ``space``, which only the step takes)"""
        return dict(eta=self.eta, norm_threshold=self.norm_threshold, momentum=self.momentum)

    def _key(self):
        return (self.eta, self.norm_threshold, self.momentum, self.space)

    def __eq__(self, other):
        return isinstance(other, APG) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"APG(eta={self.eta!r}, norm_threshold={self.norm_threshold!r}, momentum={self.momentum!r}, space={self.space!r})"


def _check_apg(apg, guidance_rescale: float = 0.0):
    apg = APG.of(apg)
    if apg is not None and apg.space == "x0" and float(guidance_rescale) > 0.0:
        raise ValueError('apg: space="x0" with guidance_rescale > 0 is not defined (the rescale is defined on the model output)')
    return apg


def compute_snr(timesteps, noise_scheduler):
    acp = noise_scheduler.alphas_cumprod
    alpha = (acp ** 0.5)[timesteps].float()
    sigma = ((1.0 - acp) ** 0.5)[timesteps].float()
    return (alpha / sigma) ** 2


def SNR_to_betas(snr):
    alpha_t = (snr / (1 + snr)) ** 0.5
    alphas_cumprod = alpha_t ** 2
    alphas = alphas_cumprod / torch.cat([torch.ones(1, device=snr.device), alphas_cumprod[:-1]])
    return 1 - alphas


class _ForwardDiffusion:
    """What the three scheduler classes share.  The trained schedule, built by the same torch ops for every class, so
    ShiftSNRScheduler's betas give bit-identical ``alphas_cumprod`` whichever class receives them; ``from_config``; the uniform
    ``previous_timestep``; the draw of a step's noise.  And diffusers' ``add_noise`` / ``get_velocity`` (the forward process
    q(x_t | x_0) of the scheduler's own ``alphas_cumprod``) through ``mvd_op_add_noise``: one fused pass, the per-sample
    coefficients looked up on the device."""

    init_noise_sigma = 1.0

    def _init_schedule(self, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas):
        if trained_betas is not None:
            self.betas = torch.as_tensor(np.asarray(trained_betas), dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(f"unsupported beta_schedule {beta_schedule}")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)

    @classmethod
    def from_config(cls, config: Any, **overrides):
        d = dict(vars(config)) if not isinstance(config, dict) else dict(config)
        d.update(overrides)
        return cls(**d)

    def previous_timestep(self, t: int) -> int:
        n = self.num_inference_steps or self.config.num_train_timesteps
        return t - self.config.num_train_timesteps // n

    @staticmethod
    def _step_noise(sample, sigma, noise, generator):
        """The noise of one step: the caller's, or, when the step has a noise term and the caller gave none, a draw from
        ``generator`` (torch's global RNG of the sample's device when None)."""
        if noise is None and sigma != 0.0:
            noise = torch.randn(sample.shape, generator=generator, device=sample.device, dtype=torch.float32)
        return noise

    def noise_tables(self, device):
        """(sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)) as fp32 vectors on ``device``: built once per (scheduler, device)."""
        device = torch.device(device)
        cache = self.__dict__.setdefault("_noise_tables", {})
        if device not in cache:
            acp = self.alphas_cumprod.to(torch.float32)
            cache[device] = ((acp ** 0.5).to(device).contiguous(), ((1.0 - acp) ** 0.5).to(device).contiguous())
        return cache[device]

    def _forward_diffusion(self, x0, noise, timesteps, velocity: bool):
        from . import ops
        from ._lib import MvdError
        if not (isinstance(x0, torch.Tensor) and isinstance(noise, torch.Tensor) and x0.is_cuda and noise.is_cuda):
            raise MvdError("add_noise / get_velocity run on the GPU only (mvd_op_add_noise): pass CUDA tensors; there is no CPU path")
        if not (isinstance(timesteps, torch.Tensor) and timesteps.is_cuda):        # host-side values: checked here
            host = torch.as_tensor(timesteps)
            T = int(self.alphas_cumprod.shape[0])
            if host.is_floating_point() or host.numel() == 0 or int(host.min()) < 0 or int(host.max()) >= T:
                raise ValueError(f"timesteps must be integers in [0, {T - 1}]")
        a, s = self.noise_tables(x0.device)
        noisy, vel = ops.add_noise(x0.to(torch.float32).contiguous(), noise.to(torch.float32).contiguous(), timesteps, a, s,
                                   noisy=not velocity, velocity=velocity)
        return vel if velocity else noisy

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps) -> torch.Tensor:
        """sqrt(acp_t) * original_samples + sqrt(1 - acp_t) * noise, one timestep per row of the batch (fp32, on the GPU).
        ``timesteps``: an int64 / int32 tensor or a list.  Values that live on the host are range-checked; a DEVICE tensor is
        not (that would synchronise): the kernel clamps it into the table for address safety only."""
        return self._forward_diffusion(original_samples, noise, timesteps, False)

    def get_velocity(self, sample: torch.Tensor, noise: torch.Tensor, timesteps) -> torch.Tensor:
        """sqrt(acp_t) * noise - sqrt(1 - acp_t) * sample (the v-prediction target); arguments as ``add_noise``."""
        return self._forward_diffusion(sample, noise, timesteps, True)


class DDPMScheduler(_ForwardDiffusion):
    """Minimal DDPM scheduler with the diffusers attribute names the reference touches."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", trained_betas=None, prediction_type: str = "v_prediction",
                 variance_type: str = "fixed_small", clip_sample: bool = False, timestep_spacing: str = "leading",
                 steps_offset: int = 0, **_ignored):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      variance_type=variance_type, clip_sample=clip_sample,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset)
        self._init_schedule(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        if variance_type != "fixed_small" or clip_sample:
            raise ValueError("only variance_type='fixed_small' without sample clipping is implemented (SD-2.1 config)")

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        if self.config.timestep_spacing == "leading":
            ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        elif self.config.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        else:
            raise ValueError(f"unsupported timestep_spacing {self.config.timestep_spacing}")
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def step_coefficients(self, t: int):
        """(c_x0_from_out, c_x0_from_sample, c_prev_from_x0, c_prev_from_sample, sigma) for one DDPM step:
        x0 = c0*model_out + c1*sample ; prev = c2*x0 + c3*sample + sigma*noise."""
        t = int(t)
        prev_t = self.previous_timestep(t)
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else 1.0
        b_t, b_prev = 1.0 - a_t, 1.0 - a_prev
        cur_alpha = a_t / a_prev
        cur_beta = 1.0 - cur_alpha
        if self.config.prediction_type == "epsilon":
            c0, c1 = -(b_t ** 0.5) / (a_t ** 0.5), 1.0 / (a_t ** 0.5)
        elif self.config.prediction_type == "v_prediction":
            c0, c1 = -(b_t ** 0.5), a_t ** 0.5
        else:
            raise ValueError(f"unsupported prediction_type {self.config.prediction_type}")
        c2 = (a_prev ** 0.5) * cur_beta / b_t
        c3 = (cur_alpha ** 0.5) * b_prev / b_t
        var = max(b_prev / b_t * cur_beta, 1e-20)
        sigma = var ** 0.5 if t > 0 else 0.0
        return c0, c1, c2, c3, sigma

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator: Optional[torch.Generator] = None,
             noise: Optional[torch.Tensor] = None):
        """One ancestral DDPM step on the GPU (fused HIP kernel); returns an object with ``prev_sample``."""
        from . import ops
        c0, c1, c2, c3, sigma = self.step_coefficients(int(timestep))
        prev = ops.ddpm_step(model_output, sample, self._step_noise(sample, sigma, noise, generator), c0, c1, c2, c3, sigma)
        return SimpleNamespace(prev_sample=prev)

    def step_guided_rescaled(self, uncond_cond: torch.Tensor, guidance_scale: float, guidance_rescale: float, timestep,
                             sample: torch.Tensor, noise: Optional[torch.Tensor] = None,
                             generator: Optional[torch.Generator] = None):
        """``step`` of the guided, rescaled model output (``ops.cfg_rescale`` of [uncond | cond] stacked on the batch dim) in ONE
        launch: the DDPM step is the samplers' affine form with r = 0.  Named apart from the samplers' ``step_guided`` on purpose:
        this class has none, so the plain guided DDPM loop stays ``cfg_combine`` + ``step``."""
        from . import ops
        _check_rescale(guidance_rescale)
        c0, c1, c2, c3, sigma = self.step_coefficients(int(timestep))
        noise = self._step_noise(sample, sigma, noise, generator)
        prev = ops.sampler_step_rescaled(uncond_cond, sample, guidance_scale, guidance_rescale, c0, c1, c3, c2, 0.0, sigma,
                                         noise=noise if sigma != 0.0 else None)
        return SimpleNamespace(prev_sample=prev)

    def step_guided_apg(self, uncond_cond: torch.Tensor, guidance_scale: float, apg, timestep, sample: torch.Tensor,
                        noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                        momentum_buffer: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0):
        """``step`` of the guided model output under adaptive projected guidance (``ops.apg`` of [uncond | cond] stacked on the
        batch dim, ``apg`` an ``APG`` or what ``APG.of`` takes) in ONE launch: the DDPM step is the samplers' affine form with
        r = 0.  ``momentum_buffer`` (the caller's, zero at the first step) is updated in place; required when the momentum is
        not 0.  Named apart like ``step_guided_rescaled``: the plain guided DDPM loop stays ``cfg_combine`` + ``step``."""
        from . import ops
        _check_rescale(guidance_rescale)
        apg = _check_apg(apg, guidance_rescale)
        if apg is None:
            raise ValueError("step_guided_apg: apg is required (an APG, a dict or a tuple)")
        c0, c1, c2, c3, sigma = self.step_coefficients(int(timestep))
        noise = self._step_noise(sample, sigma, noise, generator)
        prev = ops.sampler_step_apg(uncond_cond, sample, guidance_scale, c0, c1, c3, c2, 0.0, sigma, **apg.kwargs(),
                                    guidance_rescale=guidance_rescale, space=apg.space, momentum_buffer=momentum_buffer,
                                    noise=noise if sigma != 0.0 else None)
        return SimpleNamespace(prev_sample=prev)


def _check_rescale(guidance_rescale: float):
    if not 0.0 <= float(guidance_rescale) <= 1.0:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} must lie in [0, 1]")


_PREDICTION_TYPES = ("epsilon", "v_prediction")
_SPACINGS = ("leading", "linspace", "trailing")


def _unsupported(what: str):
    raise ValueError(f"{what} is not implemented (supported: epsilon / v_prediction, no clipping or thresholding, "
                     f"timestep_spacing leading / linspace / trailing); nothing is approximated")


class _SolverSchedule(_ForwardDiffusion):
    """What the DDIM and DPM-Solver++ classes share: the fp64 host copy of the trained schedule, the timestep grid of
    diffusers' ``set_timesteps`` and the launch of the step kernel."""

    order = 1                       # diffusers' attribute (one model evaluation per step)

    def _init_solver(self, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type,
                     timestep_spacing):
        if prediction_type not in _PREDICTION_TYPES:
            _unsupported(f"prediction_type={prediction_type!r}")
        if timestep_spacing not in _SPACINGS:
            _unsupported(f"timestep_spacing={timestep_spacing!r}")
        self._init_schedule(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self._acp = self.alphas_cumprod.double().numpy()       # host copy: the coefficients never touch a device tensor

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def _grid(self, n: int, extra: int) -> np.ndarray:
        """diffusers' grid of ``n`` timesteps; DPM-Solver++ (``extra`` = 1) spaces n + 1 points and drops the last."""
        T, spacing = self.config.num_train_timesteps, self.config.timestep_spacing
        if not 0 < n <= T:
            raise ValueError(f"num_inference_steps={n} must be in [1, {T}]")
        if spacing == "leading":
            ratio = T // (n + extra)
            ts = (np.arange(0, n + extra) * ratio).round()[::-1][:n].copy().astype(np.int64) + self.config.steps_offset
        elif spacing == "linspace":
            ts = np.linspace(0, T - 1, n + extra).round()[::-1][:n].copy().astype(np.int64)
        else:
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        return ts

    def _x0_coefficients(self, alpha: float, sigma_bar: float):
        """x0 = a0*model_out + a1*sample, with sample = alpha*x0 + sigma_bar*eps (alpha^2 + sigma_bar^2 = 1)."""
        if self.config.prediction_type == "epsilon":
            return -sigma_bar / alpha, 1.0 / alpha
        return -sigma_bar, alpha                                # v_prediction

    def _launch(self, model_out, guidance_scale, coeffs, sample, noise, generator, x0_prev=None, x0_out=None,
                guidance_rescale=0.0, apg=None, momentum_buffer=None):
        """One step kernel.  ``guidance_scale`` None: a plain step of ``model_out``; else a guided step of the stacked
        [uncond | cond] -- with ``guidance_rescale`` > 0 and guidance active the rescaled kernel, else (as in diffusers, where
        the argument is then ignored) exactly the call made without it.  ``apg`` with guidance active: the APG kernel (which
        takes the rescale along); without guidance it is ignored like the rescale."""
        from . import ops
        _check_rescale(guidance_rescale)
        apg = _check_apg(apg, guidance_rescale)
        a0, a1, p, q, r, sigma = coeffs
        noise = self._step_noise(sample, sigma, noise, generator) if sigma != 0.0 else None
        x0_prev = x0_prev if r != 0.0 else None
        if apg is not None and guidance_scale is not None and guidance_scale > 1.0:
            return ops.sampler_step_apg(model_out, sample, guidance_scale, a0, a1, p, q, r, sigma, **apg.kwargs(),
                                        guidance_rescale=guidance_rescale, space=apg.space, momentum_buffer=momentum_buffer,
                                        x0_prev=x0_prev, noise=noise, x0_out=x0_out)
        if guidance_rescale > 0.0 and guidance_scale is not None and guidance_scale > 1.0:
            return ops.sampler_step_rescaled(model_out, sample, guidance_scale, guidance_rescale, a0, a1, p, q, r, sigma,
                                             x0_prev=x0_prev, noise=noise, x0_out=x0_out)
        return ops.sampler_step(model_out, sample, a0, a1, p, q, r, sigma, x0_prev=x0_prev, noise=noise,
                                guidance_scale=guidance_scale, x0_out=x0_out)


class DDIMScheduler(_SolverSchedule):
    """diffusers-0.32.2 ``DDIMScheduler`` (Song et al. 2021) for epsilon / v_prediction, no sample clipping or
    thresholding, ``timestep_spacing`` leading / linspace / trailing with ``steps_offset``, ``set_alpha_to_one``, and
    ``eta`` as a ``step`` keyword (0: deterministic; 1: the DDPM posterior).  Defaults are SD-2.1's betas and
    v_prediction, as ``DDPMScheduler`` here.  Fields of other schedulers' configs (``variance_type``, ...) are ignored."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", trained_betas=None, clip_sample: bool = False,
                 set_alpha_to_one: bool = True, steps_offset: int = 0, prediction_type: str = "v_prediction",
                 thresholding: bool = False, timestep_spacing: str = "leading", rescale_betas_zero_snr: bool = False,
                 **_ignored):
        if clip_sample or thresholding or rescale_betas_zero_snr:
            _unsupported("clip_sample / thresholding / rescale_betas_zero_snr")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                                      steps_offset=steps_offset, prediction_type=prediction_type, thresholding=thresholding,
                                      timestep_spacing=timestep_spacing, rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._init_solver(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type,
                          timestep_spacing)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts = torch.from_numpy(self._grid(num_inference_steps, 0))
        self.timesteps = ts.to(device) if device is not None else ts

    def step_coefficients(self, t: int, eta: float = 0.0):
        """(a0, a1, p, q, r, sigma) of one DDIM step: x0 = a0*model_out + a1*sample ;
        prev = p*sample + q*x0 + sigma*noise (r = 0: no history).  The predicted noise is written as
        (sample - sqrt(a_t)*x0) / sqrt(1 - a_t), which makes the update affine in (model_out, sample, noise)."""
        t = int(t)
        prev_t = self.previous_timestep(t)
        a_t = float(self._acp[t])
        a_prev = float(self._acp[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        b_t, b_prev = 1.0 - a_t, 1.0 - a_prev
        variance = (b_prev / b_t) * (1.0 - a_t / a_prev)
        std = float(eta) * math.sqrt(max(variance, 0.0))
        a0, a1 = self._x0_coefficients(math.sqrt(a_t), math.sqrt(b_t))
        c_dir = math.sqrt(max(b_prev - std * std, 0.0))         # coefficient of the predicted noise
        p = c_dir / math.sqrt(b_t)
        q = math.sqrt(a_prev) - c_dir * math.sqrt(a_t) / math.sqrt(b_t)
        return a0, a1, p, q, 0.0, std

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0,
             use_clipped_model_output: bool = False, generator: Optional[torch.Generator] = None,
             variance_noise: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """One DDIM step on the GPU (one fused HIP kernel); returns an object with ``prev_sample``.  For eta > 0 the noise
        is ``noise`` / ``variance_noise`` or a draw from ``generator`` (torch's global RNG when None)."""
        if use_clipped_model_output:
            _unsupported("use_clipped_model_output")
        c = self.step_coefficients(int(timestep), eta)
        nz = noise if noise is not None else variance_noise
        return SimpleNamespace(prev_sample=self._launch(model_output, None, c, sample, nz, generator))

    def step_guided(self, uncond_cond: torch.Tensor, guidance_scale: float, timestep, sample: torch.Tensor,
                    noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, eta: float = 0.0,
                    guidance_rescale: float = 0.0, apg=None, momentum_buffer: Optional[torch.Tensor] = None):
        """``step`` of uncond + guidance_scale*(cond - uncond), [uncond | cond] stacked on the batch dim: ONE launch.
        ``guidance_rescale`` > 0 (with ``guidance_scale`` > 1): the guided output is rescaled per row first, in the same launch.
        ``apg`` (an ``APG``, or what ``APG.of`` takes; with ``guidance_scale`` > 1): adaptive projected guidance in place of the
        plain combine, in the same launch; ``momentum_buffer`` is the caller's (zero at the first step, updated in place),
        required when the momentum is not 0."""
        c = self.step_coefficients(int(timestep), eta)
        kw = {"apg": apg, "momentum_buffer": momentum_buffer} if apg is not None else {}
        return SimpleNamespace(prev_sample=self._launch(uncond_cond, guidance_scale, c, sample, noise, generator,
                                                        guidance_rescale=guidance_rescale, **kw))


class DPMSolverMultistepScheduler(_SolverSchedule):
    """diffusers-0.32.2 ``DPMSolverMultistepScheduler`` (Lu et al. 2022) for ``algorithm_type="dpmsolver++"`` (data
    prediction), ``solver_order`` 1 / 2, ``solver_type`` midpoint / heun, ``final_sigmas_type="zero"``, epsilon /
    v_prediction, ``timestep_spacing`` leading / linspace / trailing with ``steps_offset``, ``lower_order_final`` /
    ``euler_at_final``.  Defaults are SD-2.1's betas and v_prediction, as ``DDPMScheduler`` here.  The sigmas are kept
    in float64 (diffusers rounds them to float32: a relative difference below 1e-7).

    The multistep history (the previous step's x0) is one device buffer per (shape, device), written in place by the
    step kernel; ``set_timesteps`` resets the step index and the history."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", trained_betas=None, solver_order: int = 2,
                 prediction_type: str = "v_prediction", thresholding: bool = False, algorithm_type: str = "dpmsolver++",
                 solver_type: str = "midpoint", lower_order_final: bool = True, euler_at_final: bool = False,
                 use_karras_sigmas: bool = False, use_exponential_sigmas: bool = False, use_beta_sigmas: bool = False,
                 use_lu_lambdas: bool = False, final_sigmas_type: str = "zero", lambda_min_clipped: float = -float("inf"),
                 variance_type: Optional[str] = None, timestep_spacing: str = "linspace", steps_offset: int = 0,
                 rescale_betas_zero_snr: bool = False, **_ignored):
        if algorithm_type != "dpmsolver++":
            _unsupported(f"algorithm_type={algorithm_type!r}")
        if solver_order not in (1, 2):
            _unsupported(f"solver_order={solver_order}")
        if solver_type not in ("midpoint", "heun"):
            _unsupported(f"solver_type={solver_type!r}")
        if thresholding or use_karras_sigmas or use_exponential_sigmas or use_beta_sigmas or use_lu_lambdas:
            _unsupported("thresholding / Karras, exponential, beta sigmas / Lu lambdas")
        if final_sigmas_type != "zero" or lambda_min_clipped != -float("inf") or rescale_betas_zero_snr:
            _unsupported("final_sigmas_type != 'zero' / lambda_min_clipped / rescale_betas_zero_snr")
        if variance_type in ("learned", "learned_range"):
            _unsupported(f"variance_type={variance_type!r}")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order, prediction_type=prediction_type,
                                      thresholding=thresholding, algorithm_type=algorithm_type, solver_type=solver_type,
                                      lower_order_final=lower_order_final, euler_at_final=euler_at_final,
                                      use_karras_sigmas=use_karras_sigmas, use_exponential_sigmas=use_exponential_sigmas,
                                      use_beta_sigmas=use_beta_sigmas, use_lu_lambdas=use_lu_lambdas,
                                      final_sigmas_type=final_sigmas_type, lambda_min_clipped=lambda_min_clipped,
                                      variance_type=variance_type, timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._init_solver(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type,
                          timestep_spacing)
        self.sigmas = None
        self._hist = {}             # (shape, device) -> the x0 history buffer
        self._hist_key = None       # the buffer the previous step of this schedule wrote
        self._step_index = None
        self.lower_order_nums = 0

    @property
    def step_index(self):
        return self._step_index

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps=None):
        """The spaced grid of ``num_inference_steps`` timesteps, or an explicit integer grid ``timesteps``."""
        if (num_inference_steps is None) == (timesteps is None):
            raise ValueError("pass exactly one of num_inference_steps / timesteps")
        T = self.config.num_train_timesteps
        if timesteps is not None:
            ts = np.asarray(timesteps).astype(np.int64)
            if ts.ndim != 1 or ts.size == 0 or ts.min() < 0 or ts.max() >= T:
                raise ValueError(f"timesteps must be a non-empty 1-D grid in [0, {T - 1}]")
        else:
            ts = self._grid(int(num_inference_steps), 1)
        acp = self._acp[ts]
        self._sig = [float(s) for s in np.sqrt((1.0 - acp) / acp)] + [0.0]       # final_sigmas_type "zero"
        self.sigmas = torch.tensor(self._sig, dtype=torch.float64)
        self.timesteps = torch.from_numpy(ts.copy())
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self._ts_host = ts.tolist()
        self.num_inference_steps = len(ts)
        self._step_index = None
        self.lower_order_nums = 0
        self._hist_key = None

    def _order(self, i: int, lower_order_nums: int) -> int:
        n = len(self._ts_host)
        lower_final = i == n - 1 and (self.config.euler_at_final or (self.config.lower_order_final and n < 15)
                                      or self.config.final_sigmas_type == "zero")
        return 1 if self.config.solver_order == 1 or lower_order_nums < 1 or lower_final else 2

    def step_coefficients(self, step_index: int, order: Optional[int] = None):
        """(a0, a1, p, q, r, sigma) of step ``step_index``: x0 = a0*model_out + a1*sample ;
        prev = p*sample + q*x0 + r*x0_prev (sigma = 0).  ``order`` defaults to the one a run from step 0 uses."""
        if self.sigmas is None:
            raise ValueError("call set_timesteps first")
        i = int(step_index)
        if order is None:
            order = self._order(i, min(i, self.config.solver_order))
        lam = lambda a, sb: math.inf if sb == 0.0 else math.log(a) - math.log(sb)      # noqa: E731
        s0, st = self._sig[i], self._sig[i + 1]
        alpha_s0 = 1.0 / math.sqrt(s0 * s0 + 1.0)
        alpha_t = 1.0 / math.sqrt(st * st + 1.0)
        sb_s0, sb_t = s0 * alpha_s0, st * alpha_t
        a0, a1 = self._x0_coefficients(alpha_s0, sb_s0)
        h = lam(alpha_t, sb_t) - lam(alpha_s0, sb_s0)
        em1 = math.expm1(-h)                                    # e^{-h} - 1 (-1 at the zero final sigma, h = +inf)
        p, q, r = sb_t / sb_s0, -alpha_t * em1, 0.0
        if order == 2:
            if st == 0.0:
                raise ValueError("a second-order step onto the zero final sigma is undefined (diffusers takes order 1 there)")
            s1 = self._sig[i - 1]
            alpha_s1 = 1.0 / math.sqrt(s1 * s1 + 1.0)
            r0 = (lam(alpha_s0, sb_s0) - lam(alpha_s1, s1 * alpha_s1)) / h
            if self.config.solver_type == "midpoint":           # - 1/2 alpha_t (e^{-h} - 1) D1,  D1 = (x0 - x0_prev) / r0
                c = -0.5 * alpha_t * em1 / r0
            else:                                               # + alpha_t ((e^{-h} - 1)/h + 1) D1
                c = alpha_t * (em1 / h + 1.0) / r0
            q, r = q + c, -c
        return a0, a1, p, q, r, 0.0

    def _step(self, model_output, guidance_scale, timestep, sample, guidance_rescale: float = 0.0, apg=None, momentum_buffer=None):
        if self.sigmas is None:
            raise ValueError("call set_timesteps first")
        if self._step_index is None:                           # diffusers' index_for_timestep
            hits = [k for k, v in enumerate(self._ts_host) if v == int(timestep)]
            self._step_index = len(self._ts_host) - 1 if not hits else hits[1] if len(hits) > 1 else hits[0]
        i = self._step_index
        if i >= len(self._ts_host):
            raise ValueError("step called more often than the schedule has timesteps: call set_timesteps again")
        c = self.step_coefficients(i, self._order(i, self.lower_order_nums))
        key = (tuple(sample.shape), sample.device)
        hist = None
        if self.config.solver_order > 1:
            hist = self._hist.get(key)
            if hist is None:
                hist = self._hist[key] = torch.empty(sample.shape, device=sample.device, dtype=torch.float32)
        if c[4] != 0.0 and self._hist_key != key:
            raise ValueError("a second-order step needs the previous step's x0 of the same shape and device")
        # (the keywords go only with a rescale / APG: a stand-in for ``_launch`` of its leading parameters alone keeps working)
        out = self._launch(model_output, guidance_scale, c, sample, None, None, x0_prev=hist, x0_out=hist,
                           **({"guidance_rescale": guidance_rescale} if guidance_rescale else {}),
                           **({"apg": apg, "momentum_buffer": momentum_buffer} if apg is not None else {}))
        self._hist_key = key if hist is not None else None
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        self._step_index = i + 1
        return out

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator: Optional[torch.Generator] = None,
             noise: Optional[torch.Tensor] = None, variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """One DPM-Solver++ step on the GPU (one fused HIP kernel, which also stores this step's x0 for the next);
        returns an object with ``prev_sample``.  Deterministic: ``generator`` / ``noise`` are accepted and unused."""
        return SimpleNamespace(prev_sample=self._step(model_output, None, timestep, sample))

    def step_guided(self, uncond_cond: torch.Tensor, guidance_scale: float, timestep, sample: torch.Tensor,
                    noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                    guidance_rescale: float = 0.0, apg=None, momentum_buffer: Optional[torch.Tensor] = None):
        """``step`` of uncond + guidance_scale*(cond - uncond), [uncond | cond] stacked on the batch dim: ONE launch.
        ``guidance_rescale`` > 0 (with ``guidance_scale`` > 1): the guided output is rescaled per row first, in the same launch.
        ``apg`` / ``momentum_buffer``: as ``DDIMScheduler.step_guided``."""
        return SimpleNamespace(prev_sample=self._step(uncond_cond, guidance_scale, timestep, sample, guidance_rescale, apg,
                                                      momentum_buffer))


class UniPCCoefficients(NamedTuple):
    """The scalars of one ``mvd_op_unipc_step`` launch: x0 = a0*m + a1*x ; xc = cx*xl + c0*h0 + c1*h1 + c2*h2 + ct*x0 when ``corr``,
    else x ; y = px*xc + p0*x0 + p1*h0 + p2*h1 (xl: the previous step's corrected sample; h0, h1, h2: the previous x0 predictions,
    newest first)."""
    a0: float
    a1: float
    corr: bool
    cx: float
    c0: float
    c1: float
    c2: float
    ct: float
    px: float
    p0: float
    p1: float
    p2: float


class UniPCMultistepScheduler(_SolverSchedule):
    """diffusers-0.32.2 ``UniPCMultistepScheduler`` (Zhao et al., NeurIPS 2023) for ``predict_x0=True`` (data prediction),
    ``solver_order`` 1 / 2 / 3, ``solver_type`` bh2 / bh1, epsilon / v_prediction, ``lower_order_final``, ``disable_corrector`` (step
    indices after which no corrector runs), ``timestep_spacing`` leading / linspace / trailing with ``steps_offset``,
    ``final_sigmas_type="zero"``.  Defaults are SD-2.1's betas and v_prediction, as ``DDPMScheduler`` here; the grid is
    DPM-Solver++'s; the sigmas are kept in float64.  Unpinned against diffusers (absent here); pinned by the textbook restatement
    tests/unipc_ref.py and by identities (tests/test_unipc_cpu.py: UniP order 2 bh2 IS DPM-Solver++ 2M midpoint).

    Call i corrects the sample the previous call predicted (UniC, from sigma_{i-1} to sigma_i, with this call's model output) and
    predicts the next one (UniP, from sigma_i to sigma_{i+1}).  Both are affine in (model output, sample, last sample, x0 history),
    so a call is ONE launch (``mvd_op_unipc_step``) whose coefficients ``step_coefficients`` computes on the host in fp64.  The
    state is ``solver_order`` x0 buffers and one last-sample buffer per (shape, device); the history rotates by rotating the
    buffers' roles, the kernel writes the newest x0 into the oldest slot.  ``set_timesteps`` resets everything."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", trained_betas=None, solver_order: int = 2,
                 prediction_type: str = "v_prediction", thresholding: bool = False, predict_x0: bool = True,
                 solver_type: str = "bh2", lower_order_final: bool = True, disable_corrector=(), solver_p=None,
                 use_karras_sigmas: bool = False, use_exponential_sigmas: bool = False, use_beta_sigmas: bool = False,
                 timestep_spacing: str = "linspace", steps_offset: int = 0, final_sigmas_type: str = "zero",
                 rescale_betas_zero_snr: bool = False, **_ignored):
        if solver_order not in (1, 2, 3):
            _unsupported(f"UniPC solver_order={solver_order}")
        if solver_type not in ("bh1", "bh2"):
            _unsupported(f"UniPC solver_type={solver_type!r}")
        if not predict_x0:
            _unsupported("UniPC predict_x0=False")
        if solver_p is not None:
            _unsupported("UniPC solver_p")
        if thresholding or use_karras_sigmas or use_exponential_sigmas or use_beta_sigmas:
            _unsupported("UniPC thresholding / Karras, exponential, beta sigmas")
        if final_sigmas_type != "zero" or rescale_betas_zero_snr:
            _unsupported("UniPC final_sigmas_type != 'zero' / rescale_betas_zero_snr")
        disable_corrector = sorted({int(v) for v in disable_corrector})
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order, prediction_type=prediction_type,
                                      thresholding=thresholding, predict_x0=predict_x0, solver_type=solver_type,
                                      lower_order_final=lower_order_final, disable_corrector=disable_corrector, solver_p=solver_p,
                                      use_karras_sigmas=use_karras_sigmas, use_exponential_sigmas=use_exponential_sigmas,
                                      use_beta_sigmas=use_beta_sigmas, timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      final_sigmas_type=final_sigmas_type, rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._init_solver(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type,
                          timestep_spacing)
        self.disable_corrector = disable_corrector
        self.sigmas = None
        self._bufs = {}             # (shape, device) -> ([x0 buffers, newest first], the last-sample buffer)
        self._state_key = None      # the buffers the previous step of this schedule wrote
        self._step_index = None
        self.lower_order_nums = 0
        self.this_order = 0         # the predictor order of the previous step: the order of the next corrector

    @property
    def step_index(self):
        return self._step_index

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps=None):
        """The spaced grid of ``num_inference_steps`` timesteps, or an explicit integer grid ``timesteps``."""
        if (num_inference_steps is None) == (timesteps is None):
            raise ValueError("pass exactly one of num_inference_steps / timesteps")
        T = self.config.num_train_timesteps
        if timesteps is not None:
            ts = np.asarray(timesteps).astype(np.int64)
            if ts.ndim != 1 or ts.size == 0 or ts.min() < 0 or ts.max() >= T:
                raise ValueError(f"timesteps must be a non-empty 1-D grid in [0, {T - 1}]")
        else:
            ts = self._grid(int(num_inference_steps), 1)
        acp = self._acp[ts]
        self._sig = [float(s) for s in np.sqrt((1.0 - acp) / acp)] + [0.0]       # final_sigmas_type "zero"
        self.sigmas = torch.tensor(self._sig, dtype=torch.float64)
        self.timesteps = torch.from_numpy(ts.copy())
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self._ts_host = ts.tolist()
        self.num_inference_steps = len(ts)
        self._step_index = None
        self.lower_order_nums = 0
        self.this_order = 0
        self._state_key = None

    def _order(self, i: int, lower_order_nums: int) -> int:
        so = self.config.solver_order
        return min(so, len(self._ts_host) - i if self.config.lower_order_final else so, lower_order_nums + 1)

    def _point(self, k: int):
        """(alpha, sigma_bar, lambda) at sigma_k"""
        s = self._sig[k]
        alpha = 1.0 / math.sqrt(s * s + 1.0)
        sb = s * alpha
        return alpha, sb, (math.inf if sb == 0.0 else math.log(alpha) - math.log(sb))

    def _update(self, s0: int, order: int, corrector: bool):
        """One UniP / UniC update from sigma_{s0} to sigma_{s0 + 1} of order ``order``, as (coefficient of the sample at s0,
        coefficient of m0 = the x0 at s0, [coefficients of the x0 at s0 - 1, s0 - 2, ..], coefficient of the x0 at s0 + 1 (UniC))."""
        alpha_t, sb_t, lam_t = self._point(s0 + 1)
        _, sb_s0, lam_s0 = self._point(s0)
        h = lam_t - lam_s0
        hh = -h
        phi1 = math.expm1(hh)                                   # -1 at the zero final sigma, h = +inf
        cx, c_m0 = sb_t / sb_s0, -alpha_t * phi1
        if order == 1 and not corrector:                        # UniP-1 is the DDIM step: no B(h) term
            return cx, c_m0, [], 0.0
        if sb_t == 0.0:
            raise ValueError("a UniPC step of order > 1 onto the zero final sigma is undefined (lower_order_final=True takes "
                             "order 1 there)")
        if s0 - (order - 1) < 0:
            raise ValueError(f"a UniPC update of order {order} at sigma index {s0} needs {order - 1} earlier points")
        rks = [(self._point(s0 - k)[2] - lam_s0) / h for k in range(1, order)] + [1.0]
        B = phi1 if self.config.solver_type == "bh2" else hh
        R, b, h_phi_k, fact = [], [], phi1 / hh - 1.0, 1.0
        for j in range(1, order + 1):                           # diffusers' recurrence: b[j - 1] = phi_{j + 1} * j! / B
            R.append([r ** (j - 1) for r in rks])
            b.append(h_phi_k * fact / B)
            fact *= j + 1
            h_phi_k = h_phi_k / hh - 1.0 / fact
        if corrector:
            rhos = [0.5] if order == 1 else np.linalg.solve(np.array(R), np.array(b)).tolist()
        else:                                                   # rhos_p of order 2 is diffusers' literal 0.5, not the solve
            rhos = [0.5] if order == 2 else np.linalg.solve(np.array(R)[:-1, :-1], np.array(b)[:-1]).tolist()
            rhos = rhos + [0.0]
        # x_t = cx*x - alpha_t*phi1*m0 - alpha_t*B*(sum_k rho_k (m_k - m0) / r_k + rho_last (m_t - m0))
        hist = [-alpha_t * B * rho / r for rho, r in zip(rhos[:-1], rks[:-1])]
        c_t = -alpha_t * B * rhos[-1]
        return cx, c_m0 - sum(hist) - c_t, hist, c_t

    def step_coefficients(self, step_index: int, order: Optional[int] = None, corrector: Optional[bool] = None,
                          corrector_order: Optional[int] = None) -> UniPCCoefficients:
        """The ``UniPCCoefficients`` of call ``step_index``.  ``order`` (the predictor's), ``corrector`` (whether UniC runs) and
        ``corrector_order`` default to what a run from step 0 uses."""
        if self.sigmas is None:
            raise ValueError("call set_timesteps first")
        i = int(step_index)
        if not 0 <= i < len(self._ts_host):
            raise ValueError(f"step_index={i} outside the schedule of {len(self._ts_host)} steps")
        so = self.config.solver_order
        if order is None:
            order = self._order(i, min(i, so))
        if corrector is None:
            corrector = i > 0 and (i - 1) not in self.disable_corrector
        if corrector and i == 0:
            raise ValueError("the first step has no corrector")
        alpha_s0, sb_s0, _ = self._point(i)
        a0, a1 = self._x0_coefficients(alpha_s0, sb_s0)
        cx = ct = 0.0
        c = [0.0, 0.0, 0.0]
        if corrector:
            if corrector_order is None:
                corrector_order = self._order(i - 1, min(i - 1, so))
            cx, c[0], hist, ct = self._update(i - 1, int(corrector_order), True)
            c[1:1 + len(hist)] = hist
        px, p0, hist, _ = self._update(i, int(order), False)
        p = (hist + [0.0, 0.0])[:2]
        return UniPCCoefficients(a0, a1, bool(corrector), cx, c[0], c[1], c[2], ct, px, p0, p[0], p[1])

    def _launch_unipc(self, model_out, guidance_scale, c: UniPCCoefficients, sample, last, hist, xc_out, x0_out):
        """One ``mvd_op_unipc_step``.  ``guidance_scale`` None: a plain step of ``model_out``; else of the stacked [uncond | cond]."""
        from . import ops
        h = (list(hist) + [None] * 3)[:3]
        return ops.unipc_step(model_out, sample, c.a0, c.a1, c.px, c.p0, c.p1, c.p2, corr=c.corr, cx=c.cx, c0=c.c0, c1=c.c1, c2=c.c2,
                              ct=c.ct, last_sample=last, h0=h[0], h1=h[1], h2=h[2], guidance_scale=guidance_scale, xc_out=xc_out,
                              x0_out=x0_out)

    def _step(self, model_output, guidance_scale, timestep, sample):
        if self.sigmas is None:
            raise ValueError("call set_timesteps first")
        if self._step_index is None:                           # diffusers' index_for_timestep
            hits = [k for k, v in enumerate(self._ts_host) if v == int(timestep)]
            self._step_index = len(self._ts_host) - 1 if not hits else hits[1] if len(hits) > 1 else hits[0]
        i, n = self._step_index, len(self._ts_host)
        if i >= n:
            raise ValueError("step called more often than the schedule has timesteps: call set_timesteps again")
        key = (tuple(sample.shape), sample.device)
        if self._state_key is not None and self._state_key != key:
            raise ValueError("a UniPC step needs the previous steps' x0 and last sample of the same shape and device: "
                             "call set_timesteps to start a new trajectory")
        # without a previous step of this run (a first call in mid-schedule) there is no last sample: no corrector, as in diffusers
        corrector = i > 0 and (i - 1) not in self.disable_corrector and self._state_key is not None
        order = self._order(i, self.lower_order_nums)
        c = self.step_coefficients(i, order, corrector, self.this_order if corrector else None)
        if key not in self._bufs:
            new = lambda: torch.empty(sample.shape, device=sample.device, dtype=torch.float32)      # noqa: E731
            self._bufs[key] = ([new() for _ in range(self.config.solver_order)], new())
        hist, last = self._bufs[key]
        # the next call's corrector reads this call's corrected sample; where none runs, it is not written
        keep_last = i + 1 < n and i not in self.disable_corrector
        out = self._launch_unipc(model_output, guidance_scale, c, sample, last, hist, last if keep_last else None, hist[-1])
        hist.insert(0, hist.pop())                             # the slot just written is the newest: rotate the roles
        self._state_key = key
        self.this_order = order
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        self._step_index = i + 1
        return out

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator: Optional[torch.Generator] = None,
             noise: Optional[torch.Tensor] = None, variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """One UniPC call on the GPU: the corrector of the previous step and the predictor of this one in ONE fused HIP kernel,
        which also stores this step's x0 and corrected sample for the next; returns an object with ``prev_sample``.
        Deterministic: ``generator`` / ``noise`` are accepted and unused."""
        return SimpleNamespace(prev_sample=self._step(model_output, None, timestep, sample))

    def step_guided(self, uncond_cond: torch.Tensor, guidance_scale: float, timestep, sample: torch.Tensor,
                    noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                    guidance_rescale: float = 0.0, apg=None, momentum_buffer: Optional[torch.Tensor] = None):
        """``step`` of uncond + guidance_scale*(cond - uncond), [uncond | cond] stacked on the batch dim: ONE launch.  With
        ``guidance_rescale`` > 0 or ``apg`` (and ``guidance_scale`` > 1) TWO launches: ``ops.cfg_rescale`` / ``ops.apg``, then the
        unguided step.  APG in ``space="x0"`` is not offered by UniPC (its step has no x0-space entry)."""
        from . import ops
        _check_rescale(guidance_rescale)
        apg = _check_apg(apg, guidance_rescale)
        if apg is not None and apg.space == "x0":
            raise ValueError('apg: space="x0" is not implemented for UniPC (UniPCMultistepScheduler applies APG to the model output '
                             'in a launch of its own); use space="output" or another sampler')
        active = guidance_scale is not None and guidance_scale > 1.0
        if active and apg is not None:
            m = ops.apg(uncond_cond, guidance_scale, **apg.kwargs(), guidance_rescale=guidance_rescale, momentum_buffer=momentum_buffer)
            return SimpleNamespace(prev_sample=self._step(m, None, timestep, sample))
        if active and guidance_rescale > 0.0:
            m = ops.cfg_rescale(uncond_cond, guidance_scale, guidance_rescale)
            return SimpleNamespace(prev_sample=self._step(m, None, timestep, sample))
        return SimpleNamespace(prev_sample=self._step(uncond_cond, guidance_scale, timestep, sample))


class ShiftSNRScheduler:
    """/root/reference/src/training/scheduler.py:74-150."""

    def __init__(self, noise_scheduler, timesteps, shift_scale, scheduler_class):
        self.noise_scheduler, self.timesteps, self.shift_scale, self.scheduler_class = \
            noise_scheduler, timesteps, shift_scale, scheduler_class

    def _get_shift_scheduler(self):
        snr = compute_snr(self.timesteps, self.noise_scheduler)
        betas = SNR_to_betas(snr / self.shift_scale)
        return self.scheduler_class.from_config(self.noise_scheduler.config, trained_betas=betas.numpy())

    def _get_interpolated_shift_scheduler(self):
        snr = compute_snr(self.timesteps, self.noise_scheduler)
        shifted = snr / self.shift_scale
        w = self.timesteps.float() / (self.noise_scheduler.config.num_train_timesteps - 1)
        interp = torch.exp(torch.log(snr) * (1 - w) + torch.log(shifted) * w)
        return self.scheduler_class.from_config(self.noise_scheduler.config, trained_betas=SNR_to_betas(interp).numpy())

    @classmethod
    def from_scheduler(cls, noise_scheduler, shift_mode="default", timesteps=None, shift_scale=1.0, scheduler_class=None):
        if timesteps is None:
            timesteps = torch.arange(0, noise_scheduler.config.num_train_timesteps)
        if scheduler_class is None:
            scheduler_class = noise_scheduler.__class__
        s = cls(noise_scheduler, timesteps, shift_scale, scheduler_class)
        if shift_mode == "default":
            return s._get_shift_scheduler()
        if shift_mode == "interpolated":
            return s._get_interpolated_shift_scheduler()
        raise ValueError(f"Unknown shift_mode: {shift_mode}")
