"""The caller of the hot path: ``MVDPipeline.__call__`` with the signature and semantics of
/root/reference/src/models/pipeline.py:12-186 over the HIP engine, with device-resident state and no host syncs in
the loop (CFG concat -> MultiViewUNet -> CFG combine -> scheduler.step, each step a handful of kernel launches).

The reference class derives from diffusers' ``StableDiffusionPipeline`` and gets its text encoder, tokenizer and VAE
from ``from_pretrained``.  diffusers / SD-2.1 weights do not exist in this image, so this class is self-contained:

* ``unet`` (the ``MultiViewUNet`` mirror) and ``scheduler`` are always present;
* ``text_encoder`` / ``tokenizer`` / ``vae`` are optional components.  Without a text encoder the caller passes
  ``prompt_embeds`` (already a parameter of the reference signature); without a VAE the caller passes
  ``source_image_latents`` instead of ``source_images`` and asks for ``output_type="latent"``.  Asking for something a
  missing component would have to produce raises ``MvdError`` -- nothing is silently skipped.
* ``vae`` may be any object with the diffusers ``AutoencoderKL`` protocol (``encode(x).latent_dist.sample()``,
  ``decode(z).sample``, ``config.scaling_factor``); ``mvd_amd.vae.AutoencoderKLHIP`` is the engine-backed one (row N3).

Reference quirk Q7 is kept: ``ref_scale``, ``use_camera_embeddings`` and ``use_image_conditioning`` are accepted and
unused (pipeline.py:34-36, 134-135); the effective switches live on the UNet.  ``eta`` is likewise accepted and never
forwarded (pipeline.py:161 calls ``scheduler.step`` without it), so with ``sampler="ddim"`` this pipeline runs DDIM at
eta = 0; a caller who wants the stochastic form drives ``DDIMScheduler.step(..., eta=)`` directly.
"""
from __future__ import annotations

import inspect
import json
import os
from types import SimpleNamespace
from typing import Any, Callable, Dict, List, Optional, Union

import logging

import torch

from . import _lib as L
from . import ops
from .layout import ViewLayout


class MVDDenoiser:
    """The loop body of pipeline.py:119-166 starting from prompt embeddings / source latents."""

    def __init__(self, unet, scheduler):
        self.unet, self.scheduler = unet, scheduler

    @torch.no_grad()
    def __call__(self, prompt_embeds: torch.Tensor, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, latents: Optional[torch.Tensor] = None,
                 source_camera: Optional[torch.Tensor] = None, target_camera: Optional[torch.Tensor] = None,
                 source_image_latents: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                 height: int = 64, width: int = 64, noise_per_step=None, callback=None, callback_steps: int = 1,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None, views: Optional[int] = None,
                 objects: Optional[int] = None, *, guidance_rescale: float = 0.0, apg=None):
        """``guidance_rescale`` (diffusers' argument of that name; Lin et al. 2024, section 3.4): with guidance active
        (``guidance_scale > 1``) and a value in (0, 1], every row's guided output is rescaled towards the standard deviation of its
        conditional output before the scheduler step -- statistics, rescale and step in ONE launch per step for all three samplers
        (DESIGN.md section 9 N17).  0.0 (the default), or no guidance: ignored, the loop issues the launches it always did.

        ``apg`` (``mvd_amd.scheduler.APG``, or a dict / tuple ``APG.of`` takes; Sadat et al. 2025, diffusers'
        ``AdaptiveProjectedGuidance``): with guidance active, adaptive projected guidance replaces the plain combine -- projection,
        norm cap, momentum, the optional rescale and the step in ONE launch per step for all three samplers (DESIGN.md section 9
        N19).  The momentum buffer belongs to this call: allocated and zeroed here, only when the momentum is not 0.  ``None`` (the
        default), or no guidance: the loop issues the launches it always did.

        ``views`` (MVDPipeline.generate_views): ``latents`` and the target cameras hold that many rows for ONE prompt and ONE
        source row; every step is one shared-reference forward (``MultiViewUNet.forward(..., views=)``).  ``objects``
        (MVDPipeline.generate_views_batch): O prompts and O source rows, ``latents`` and the cameras O * views rows, object-major;
        every step is one object forward (``MultiViewUNet.forward(..., views=, objects=)``).  ``views`` a sequence
        ``(V_0, .., V_{O-1})``: ragged view counts -- O prompts and O source rows, ``latents`` and the cameras sum(V_o) rows,
        object-major; every step is one ragged forward (``MultiViewUNet.forward(..., views=(V_0, ..))``).

        DeepCache (``unet.enable_deepcache(cache_interval, cache_branch_id)``): step i (0-based) is a refresh
        step iff ``i % cache_interval == 0`` -- the whole UNet, which also stores its deep feature -- and a shallow step otherwise;
        under guidance the ``[uncond | cond]`` rows are one forward and share one stored feature.  Disabled, or
        ``cache_interval=1``: the loop issues the launches it always did."""
        if not 0.0 <= float(guidance_rescale) <= 1.0:
            raise ValueError(f"guidance_rescale={guidance_rescale!r} must lie in [0, 1]")
        rescale = float(guidance_rescale) if guidance_scale > 1.0 else 0.0      # without guidance it is ignored, as in diffusers
        from .scheduler import _check_apg
        apg = _check_apg(apg, guidance_rescale)
        if guidance_scale <= 1.0:                                               # without guidance there is no update to project
            apg = None
        dev = self.unet._exec_device()
        B = prompt_embeds.shape[0]
        cfg = guidance_scale > 1.0 and negative_prompt_embeds is not None       # pipeline.py:77-80
        embeds = torch.cat([negative_prompt_embeds.to(prompt_embeds.device), prompt_embeds]) if cfg else prompt_embeds
        embeds = embeds.to(dev, torch.float32)
        lay = ViewLayout.parse(views, objects)
        if lay.rows:
            # one prompt per object, one latent row per view
            if B != lay.sources:
                raise L.MvdError(f"views: one prompt for the one object, got {B} rows of prompt_embeds" if not (lay.counts or lay.objects) else
                                 f"{f'views={lay.counts}' if lay.counts else 'objects'}: one prompt per object, got {B} rows of prompt_embeds for {lay.sources} objects")
            if guidance_scale > 1.0 and not cfg:
                # the doubled latents against one text row per object, [positive x O | positive x O]: the repeat of mvd_unet.py:233-237
                embeds = embeds.repeat(2, 1, 1)
            B = lay.rows
        if latents is None:
            latents = torch.randn(B, 4, height, width, generator=generator, device=dev, dtype=torch.float32)
            latents = latents * self.scheduler.init_noise_sigma
        latents = latents.to(dev, torch.float32).contiguous()
        self.scheduler.set_timesteps(num_inference_steps)
        extra = {}
        if source_camera is not None:
            extra["source_camera"] = source_camera.to(dev)
        if target_camera is not None:
            extra["target_camera"] = target_camera.to(dev)
        if source_image_latents is not None:
            extra["source_image_latents"] = source_image_latents.to(dev)
        extra.update(lay.kwargs())
        # Q5: the reference K/V of a previous call (another object) must never be reused by this one
        if hasattr(self.unet, "reset_reference_cache"):
            self.unet.reset_reference_cache()
        guided_step = getattr(self.scheduler, "step_guided", None)              # DDIM / DPM-Solver++ (DDPM has none)
        rescaled_step = getattr(self.scheduler, "step_guided_rescaled", None)   # DDPM's guided-and-rescaled step
        # the keyword goes only with a rescale: a scheduler of the caller's whose step_guided has none keeps working without one
        guided_kw = {"guidance_rescale": rescale} if rescale > 0.0 else {}
        apg_step = None
        if apg is not None:
            # the momentum buffer is this call's own: zero at the first step, updated in place by every step's launch
            momentum = torch.zeros_like(latents) if apg.momentum != 0.0 else None
            if guided_step is not None and "apg" in inspect.signature(guided_step).parameters:
                guided_kw.update(apg=apg, momentum_buffer=momentum)
            else:
                guided_step, apg_step = None, getattr(self.scheduler, "step_guided_apg", None)  # DDPM's; else a caller's scheduler
                if apg_step is None and apg.space != "output":
                    raise L.MvdError('apg: space="x0" needs a scheduler with step_guided(..., apg=) or step_guided_apg '
                                     f"({type(self.scheduler).__name__} has neither)")
        deep = deepcache_schedule(getattr(self.unet, "deepcache", None), len(self.scheduler.timesteps))
        ts_host = self.scheduler.timesteps.tolist()                             # host ints for the scheduler's coefficients
        ts_dev = torch.tensor(ts_host, dtype=torch.float32, device=dev)         # ONE upload: a per-step scalar upload would make
        for i, t in enumerate(ts_host):                                         # the host wait for the previous step's kernels
            x_in = torch.cat([latents] * 2) if guidance_scale > 1.0 else latents  # pipeline.py:141
            out = self.unet(sample=x_in, timestep=ts_dev[i], encoder_hidden_states=embeds,
                            cross_attention_kwargs=cross_attention_kwargs, **extra,
                            **({"deep_cache": deep[i]} if deep is not None else {})).sample.float().contiguous()
            nz = None if noise_per_step is None else noise_per_step[i]
            if guidance_scale > 1.0 and guided_step is not None:
                # DDIM / DPM-Solver++: the guidance combine (pipeline.py:156-158) and the step in ONE fused launch; with guidance
                # rescale the row statistics and the rescale too
                latents = guided_step(out, guidance_scale, t, latents, noise=nz, **guided_kw).prev_sample
            elif apg_step is not None:                                          # DDPM under APG: the APG kernel (r = 0), ONE launch
                latents = apg_step(out, guidance_scale, apg, t, latents, noise=nz, momentum_buffer=momentum,
                                   guidance_rescale=rescale).prev_sample
            elif apg is not None:                                               # a scheduler of the caller's: APG, then its step
                m = ops.apg(out, guidance_scale, **apg.kwargs(), guidance_rescale=rescale, momentum_buffer=momentum)
                latents = self.scheduler.step(m, t, latents, noise=nz).prev_sample
            elif rescale > 0.0 and rescaled_step is not None:                   # DDPM: the same kernel (r = 0), ONE launch
                latents = rescaled_step(out, guidance_scale, rescale, t, latents, noise=nz).prev_sample
            elif rescale > 0.0:                                                 # a scheduler of the caller's: rescale, then its step
                latents = self.scheduler.step(ops.cfg_rescale(out, guidance_scale, rescale), t, latents, noise=nz).prev_sample
            else:
                if guidance_scale > 1.0:                                        # pipeline.py:156-158
                    out = ops.cfg_combine(out, guidance_scale)
                # pipeline.py:161 calls scheduler.step(noise_pred, t, latents) WITHOUT the generator: the ancestral noise comes
                # from torch's global RNG (of the latents' device), the caller's generator only seeds the initial latents
                latents = self.scheduler.step(out, t, latents, noise=nz).prev_sample
            if callback is not None and i % callback_steps == 0:                # pipeline.py:165-166
                callback(i, t, latents)
        return latents


def deepcache_schedule(setting, steps: int):
    """The ``deep_cache`` keyword of every step of a loop of ``steps`` steps under ``setting`` = ``(cache_interval, cache_branch_id)``:
    ``"refresh"`` where ``i % cache_interval == 0``, else ``"reuse"``.  ``None`` -- no keyword at all, the loop as it always was --
    without a setting or with ``cache_interval == 1``."""
    if setting is None or int(setting[0]) == 1:
        return None
    return ["refresh" if i % int(setting[0]) == 0 else "reuse" for i in range(steps)]


logger = logging.getLogger(__name__)


class MVDPipeline:
    """Mirror of /root/reference/src/models/pipeline.py::MVDPipeline (same ``__call__`` signature and return value)."""

    def __init__(self, unet, scheduler, vae=None, text_encoder=None, tokenizer=None, vae_scale_factor: int = 8):
        self.unet, self.scheduler = unet, scheduler
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.vae_scale_factor = vae_scale_factor
        self.safety_checker = None
        self.feature_extractor = None
        # attributes create_mvd_pipeline sets on the reference pipeline (mvd_unet.py:449-451)
        self.use_camera_conditioning = getattr(unet, "use_camera_conditioning", True)
        self.use_image_conditioning = getattr(unet, "use_image_conditioning", True)
        self.img_ref_scale = getattr(unet, "img_ref_scale", 0.3)

    # ------------------------------------------------------------------ small pieces of the diffusers base class
    @property
    def device(self) -> torch.device:
        return self.unet._exec_device() if torch.cuda.is_available() else torch.device("cpu")

    def to(self, *args, **kwargs):
        self.unet.to(*args, **kwargs)
        for m in (self.vae, self.text_encoder):
            if m is not None and hasattr(m, "to"):
                m.to(*args, **kwargs)
        return self

    def progress_bar(self, iterable):
        return iterable

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' ``StableDiffusionPipeline.enable_freeu``: FreeU on the UNet's main pass for every call that follows
        (``MultiViewUNet.enable_freeu``).  SD-2.1: ``s1=0.9, s2=0.2, b1=1.4, b2=1.6``."""
        self.unet.enable_freeu(s1, s2, b1, b2)

    def disable_freeu(self):
        self.unet.disable_freeu()

    def enable_tome(self, ratio: float = 0.5, max_downsample: int = 1):
        """``tomesd.apply_patch(pipe, ratio=, max_downsample=)``: token merging in front of the UNet's self-attention for every call
        that follows (``MultiViewUNet.enable_tome``)."""
        self.unet.enable_tome(ratio, max_downsample)

    def disable_tome(self):
        self.unet.disable_tome()

    def enable_todo(self, factor: int = 2, factor_level_2: int = 1, method: str = "nearest"):
        """Token downsampling of the UNet's self-attention keys and values (ToDo) for every call that follows -- ``__call__``,
        ``generate_views`` and ``generate_views_batch`` alike (``MultiViewUNet.enable_todo``)."""
        self.unet.enable_todo(factor, factor_level_2, method)

    def disable_todo(self):
        self.unet.disable_todo()

    def enable_deepcache(self, cache_interval: int = 3, cache_branch_id: int = 0):
        """DeepCache (``DeepCacheSDHelper``'s parameters) for every call that follows -- ``__call__``, ``generate_views`` and
        ``generate_views_batch`` alike: every ``cache_interval``-th step runs the whole UNet, the steps in between only its
        outermost layers around the deep feature that step stored (``MultiViewUNet.enable_deepcache``)."""
        self.unet.enable_deepcache(cache_interval, cache_branch_id)

    def disable_deepcache(self):
        self.unet.disable_deepcache()

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """StableDiffusionPipeline.prepare_latents: N(0,1) of the latent shape times ``init_noise_sigma``."""
        shape = (batch_size, num_channels_latents, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor)
        if isinstance(generator, (list, tuple)):
            # diffusers' prepare_latents / randn_tensor: one generator per latent (the signature's List[torch.Generator],
            # pipeline.py:22) -- a list of another length is an error, each row is drawn from its own generator
            if len(generator) != batch_size:
                raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective "
                                 f"batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
            if len(generator) == 1:
                generator = generator[0]
        if latents is None:
            if isinstance(generator, (list, tuple)):
                rows = [torch.randn((1,) + shape[1:], generator=g, device=g.device, dtype=torch.float32).to(device) for g in generator]
                latents = torch.cat(rows, dim=0)
            else:
                gdev = generator.device if isinstance(generator, torch.Generator) else device
                latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(device)
        return latents.to(device) * self.scheduler.init_noise_sigma

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        return [Image.fromarray((im * 255).round().astype("uint8")) for im in images]

    def _encode_prompt(self, prompt):
        if self.text_encoder is None or self.tokenizer is None:
            raise L.MvdError("MVDPipeline has no text encoder / tokenizer (no CLIP weights in this image): "
                             "pass prompt_embeds / negative_prompt_embeds")
        ti = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                            return_tensors="pt")
        return self.text_encoder(ti.input_ids.to(self.device))[0]

    # ------------------------------------------------------------------ the one generation path under the entry points
    def _size(self, height, width):
        side = self.unet.config.sample_size * self.vae_scale_factor            # pipeline.py:82-83
        return height or side, width or side

    def _encode_sources(self, source_images, repeat_to: int = 0):
        """``source_images`` -> ``source_image_latents`` (pipeline.py:100-117): all rows in one VAE call.  ``repeat_to``
        (``__call__`` alone): fewer source rows than that are repeated, as the reference repeats them for its prompts."""
        if self.vae is None:
            raise L.MvdError("MVDPipeline has no VAE: pass source_image_latents (scaled by the VAE scaling factor) "
                             "instead of source_images, or attach mvd_amd.vae.AutoencoderKLHIP")
        si = source_images.to(device=self.device)
        if bool(si.min() >= 0) and bool(si.max() <= 1):                          # one host sync, outside the loop
            si = 2 * si - 1
        if si.shape[0] < repeat_to:
            si = si.repeat(repeat_to // si.shape[0], 1, 1, 1)
        return self.vae.encode(si).latent_dist.sample() * self.vae.config.scaling_factor

    def _denoise(self, prompt_embeds, num_inference_steps, guidance_scale, cross_attention_kwargs=None, **kw):
        return MVDDenoiser(self.unet, self.scheduler)(prompt_embeds, num_inference_steps, guidance_scale,
                                                      cross_attention_kwargs=cross_attention_kwargs or {}, **kw)

    def _images(self, latents, output_type, return_dict):
        """The final latents as every entry point returns them: all rows in one VAE decode."""
        if output_type == "latent":
            image = latents
        else:                                                                    # pipeline.py:168-181
            if self.vae is None:
                raise L.MvdError("MVDPipeline has no VAE to decode with: use output_type='latent'")
            image = self.vae.decode(latents / self.vae.config.scaling_factor).sample
            image = (image / 2 + 0.5).clamp(0, 1)
            if output_type == "pil":
                image = self.numpy_to_pil(image.cpu().permute(0, 2, 3, 1).float().numpy())
        if not return_dict:
            return image
        return {"images": image}

    def _turntable(self, prompt_embeds, source_camera, target_camera, layout, *, who, rows, rows_of, sources, sources_of,
                   source_images, source_image_latents, height, width, generator, latents, output_type, return_dict, **loop):
        """What ``generate_views`` and both forms of ``generate_views_batch`` do once their arguments are checked and their camera
        rows built: ``rows`` latent rows (drawn, or the caller's) against ``sources`` source rows (VAE-encoded in one call, or the
        caller's latents), one denoising loop in the forward that ``layout`` (the denoiser's ``views`` / ``objects``) names, one
        decode.  ``rows_of`` / ``sources_of`` word the two row-count errors for the caller ``who``; ``loop`` goes to the denoiser
        as it is."""
        height, width = self._size(height, width)
        if latents is None:
            latents = self.prepare_latents(rows, 4, height, width, prompt_embeds.dtype, self.device, generator)
        if latents.shape[0] != rows:
            raise L.MvdError(f"{who}: {latents.shape[0]} rows of latents for {rows_of}")
        if source_images is not None:
            source_image_latents = self._encode_sources(source_images)
        if source_image_latents is None or source_image_latents.shape[0] != sources:
            raise L.MvdError(f"{who}: {sources_of}")
        latents = self._denoise(prompt_embeds, latents=latents, source_camera=source_camera, target_camera=target_camera,
                                source_image_latents=source_image_latents, **loop, **layout)
        return self._images(latents, output_type, return_dict)

    # ------------------------------------------------------------------ pipeline.py:12-186
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 latents: Optional[torch.FloatTensor] = None, prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_prompt_embeds: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
                 callback_steps: int = 1, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 source_camera: Optional[torch.Tensor] = None, target_camera: Optional[torch.Tensor] = None,
                 source_images: Optional[torch.Tensor] = None, ref_scale: float = 0.1, use_camera_embeddings: bool = True,
                 use_image_conditioning: bool = True, debug_log_file_path: Optional[str] = None, *,
                 source_image_latents: Optional[torch.Tensor] = None, noise_per_step=None,
                 guidance_rescale: float = 0.0, apg=None):
        dev = self.device
        if prompt is not None and isinstance(prompt, str):                       # :45-50
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        elif prompt_embeds is not None:
            batch_size = prompt_embeds.shape[0]
        else:
            raise L.MvdError("MVDPipeline: neither prompt nor prompt_embeds given")
        if prompt_embeds is None:                                                # :52-62
            prompt_embeds = self._encode_prompt(prompt if prompt is not None else "")
        if negative_prompt_embeds is None and negative_prompt is not None:       # :64-75
            negative_prompt_embeds = self._encode_prompt(negative_prompt)

        height, width = self._size(height, width)                                # :82-83
        if latents is None:                                                      # :85-95
            latents = self.prepare_latents(batch_size * num_images_per_prompt, 4, height, width, prompt_embeds.dtype, dev,
                                           generator)

        if source_images is not None:                                            # :100-117
            source_image_latents = self._encode_sources(source_images, repeat_to=batch_size)

        latents = self._denoise(prompt_embeds, num_inference_steps, guidance_scale, negative_prompt_embeds=negative_prompt_embeds,
                                latents=latents, source_camera=source_camera, target_camera=target_camera,
                                source_image_latents=source_image_latents,
                                generator=generator if isinstance(generator, torch.Generator) else None,
                                noise_per_step=noise_per_step, callback=callback, callback_steps=callback_steps,
                                cross_attention_kwargs=cross_attention_kwargs, guidance_rescale=guidance_rescale,
                                **({"apg": apg} if apg is not None else {}))
        return self._images(latents, output_type, return_dict)

    @torch.no_grad()
    def generate_views(self, prompt: Optional[str] = None, source_images: Optional[torch.Tensor] = None,
                       source_camera: Optional[torch.Tensor] = None, target_cameras: Optional[torch.Tensor] = None,
                       height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                       guidance_scale: float = 7.5, negative_prompt: Optional[str] = None,
                       generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                       latents: Optional[torch.FloatTensor] = None, prompt_embeds: Optional[torch.FloatTensor] = None,
                       negative_prompt_embeds: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                       return_dict: bool = True, callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
                       callback_steps: int = 1, cross_attention_kwargs: Optional[Dict[str, Any]] = None, *,
                       source_image_latents: Optional[torch.Tensor] = None, noise_per_step=None,
                       guidance_rescale: float = 0.0, apg=None):
        """V views of ONE object from one source image: what V calls ``pipe(prompt, source_images=, source_camera=,
        target_camera=target_cameras[v:v+1], ...)`` give (the loop of infer.py:111-122, a turntable), in one denoising loop whose
        every step is ONE shared-reference forward: the prompt is encoded once, the source VAE-encoded
        once, the reference encoder pass and its K/V exist once per step (once per call with ``unet.cache_reference``), the V
        latents are decoded in one VAE call.  Not a method of the reference's pipeline.

        ``target_cameras``: (V, 3|4, 4), e.g. ``mvd_amd.utils.orbit_cameras(V)``; ``source_camera``: (3|4, 4) or (1, 3|4, 4);
        ``source_images`` / ``source_image_latents``: ONE row.  ``generator``: one generator (the V initial latents are one draw of
        (V, 4, h, w)) or a list of V (row v is view v's own draw -- equal to the latents of the per-view call with
        ``generator[v]``); ``latents``: V rows.  Returns V images (or latents) like ``__call__``.

        Ancestral noise (``sampler="ddpm"``): like ``__call__``, the step noise comes from torch's global RNG unless
        ``noise_per_step`` is given -- here ONE draw of (V, 4, h, w) per step, where V separate calls make V draws of (1, 4, h, w)
        in call-major order.  The two streams differ, so DDPM results equal the per-view calls' only through
        ``noise_per_step[i]`` = (V, 4, h, w) whose row v is what view v's call gets as ``noise_per_step[i]``; DDIM (eta 0) and
        DPM-Solver++ take no step noise.  The camera encoder's per-call random projection (Q1) is drawn once per forward for all
        views; the per-view calls draw one each unless ``unet.fourier_projection`` pins it."""
        if target_cameras is None or target_cameras.dim() != 3:
            raise L.MvdError("generate_views: target_cameras must be (V, 3|4, 4)")
        V = target_cameras.shape[0]
        if isinstance(prompt, (list, tuple)):
            raise L.MvdError("generate_views: one prompt (a str) for the one object")
        if prompt is None and prompt_embeds is None:
            raise L.MvdError("MVDPipeline: neither prompt nor prompt_embeds given")
        if prompt_embeds is None:
            prompt_embeds = self._encode_prompt(prompt)                           # once for all views
        if negative_prompt_embeds is None and negative_prompt is not None:
            negative_prompt_embeds = self._encode_prompt(negative_prompt)
        if prompt_embeds.shape[0] != 1:
            raise L.MvdError(f"generate_views: one prompt for the one object, got {prompt_embeds.shape[0]} rows of prompt_embeds")
        if source_camera is None:
            raise L.MvdError("generate_views: source_camera is required")
        src = source_camera if source_camera.dim() == 3 else source_camera.unsqueeze(0)
        if src.shape[0] != 1 or src.shape[1:] != target_cameras.shape[1:]:
            raise L.MvdError(f"generate_views: source_camera {tuple(source_camera.shape)} vs target_cameras {tuple(target_cameras.shape)}")
        return self._turntable(
            prompt_embeds, src.expand(V, -1, -1), target_cameras, dict(views=V), who="generate_views",
            rows=V, rows_of=f"{V} target cameras",
            sources=1, sources_of="ONE source image (source_images or source_image_latents with one row)",
            source_images=source_images, source_image_latents=source_image_latents, height=height, width=width, generator=generator,
            latents=latents, output_type=output_type, return_dict=return_dict, num_inference_steps=num_inference_steps,
            guidance_scale=guidance_scale, negative_prompt_embeds=negative_prompt_embeds, noise_per_step=noise_per_step,
            callback=callback, callback_steps=callback_steps, cross_attention_kwargs=cross_attention_kwargs,
            guidance_rescale=guidance_rescale, **({"apg": apg} if apg is not None else {}))

    @torch.no_grad()
    def generate_views_batch(self, prompts: Optional[List[str]] = None, source_images: Optional[torch.Tensor] = None,
                             source_cameras: Optional[torch.Tensor] = None, target_cameras: Optional[torch.Tensor] = None,
                             height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                             guidance_scale: float = 7.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                             generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                             latents: Optional[torch.FloatTensor] = None, prompt_embeds: Optional[torch.FloatTensor] = None,
                             negative_prompt_embeds: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                             return_dict: bool = True, callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
                             callback_steps: int = 1, cross_attention_kwargs: Optional[Dict[str, Any]] = None, *,
                             source_image_latents: Optional[torch.Tensor] = None, noise_per_step=None,
                             guidance_rescale: float = 0.0, apg=None):
        """Turntables of O objects, V views each: what O calls of ``generate_views`` (O * V calls of ``pipe(...)``) give, in one
        denoising loop whose every step is ONE object forward.  The prompts are encoded once, the O
        sources VAE-encoded in one call, the reference encoder pass runs at batch O (once per call with
        ``unet.cache_reference``) with per-object statistics, the O * V latents are decoded in one VAE call.  Not a method of
        the reference's pipeline.

        ``prompts``: a list of O strings, or ``prompt_embeds`` with O rows (``negative_prompt``: one string for all or a list of O;
        ``negative_prompt_embeds``: 1 or O rows); ``source_images`` / ``source_image_latents``: O rows; ``source_cameras``:
        (O, 3|4, 4); ``target_cameras``: (O, V, 3|4, 4), or (V, 3|4, 4) for every object.  Every object has the same V.
        ``generator``: one generator (the initial latents are one draw of (O V, 4, h, w)) or a list of O * V (row o * V + v is that
        view's own draw); ``latents``: O * V rows, object-major.  Returns O * V images (or latents) in object-major order.

        Ancestral noise (``sampler="ddpm"``): ONE draw of (O V, 4, h, w) per step from torch's global RNG, or ``noise_per_step[i]``
        of that shape (row o * V + v is what that view's own call gets).  The camera encoder's random projection (Q1) is drawn
        once per forward for all rows.

        Ragged view counts: ``target_cameras`` a LIST of O tensors ``(V_o, 3|4, 4)``, V_o >= 1 -- object o
        gets V_o views, R = sum V_o.  Prompts, sources and source cameras stay one per object; ``latents``, a generator list,
        ``noise_per_step[i]`` and the returned images have R rows, object-major (row sum(V_0 .. V_{o-1}) + v); every step is one
        ragged forward, which is the R independent calls.  Equal counts give what the tensor form gives, bit for bit."""
        if prompts is not None and (isinstance(prompts, str) or not isinstance(prompts, (list, tuple))):
            raise L.MvdError("generate_views_batch: prompts must be a list of strings, one per object")
        if prompts is None and prompt_embeds is None:
            raise L.MvdError("MVDPipeline: neither prompts nor prompt_embeds given")
        if prompt_embeds is None:
            prompt_embeds = self._encode_prompt(list(prompts))                    # once for all objects and views
        O = prompt_embeds.shape[0]
        if prompts is not None and len(prompts) != O:
            raise L.MvdError(f"generate_views_batch: {len(prompts)} prompts vs {O} rows of prompt_embeds")
        if negative_prompt_embeds is None and negative_prompt is not None:
            neg = [negative_prompt] * O if isinstance(negative_prompt, str) else list(negative_prompt)
            if len(neg) != O:
                raise L.MvdError(f"generate_views_batch: {len(neg)} negative prompts for {O} objects")
            negative_prompt_embeds = self._encode_prompt(neg)
        if negative_prompt_embeds is not None:
            if negative_prompt_embeds.shape[0] == 1:
                negative_prompt_embeds = negative_prompt_embeds.expand(O, -1, -1)
            if negative_prompt_embeds.shape[0] != O:
                raise L.MvdError(f"generate_views_batch: {negative_prompt_embeds.shape[0]} rows of negative_prompt_embeds for {O} objects")
        def check_source_cameras(cam_shape):
            if source_cameras is None or source_cameras.dim() != 3 or source_cameras.shape[0] != O or source_cameras.shape[1:] != cam_shape:
                raise L.MvdError(f"generate_views_batch: source_cameras must be ({O}, {cam_shape[0]}, 4), one per object")

        # the camera rows, object-major: an object's source camera on each of its views' rows
        if isinstance(target_cameras, (list, tuple)):                             # ragged: one (V_o, 3|4, 4) tensor per object
            cams = list(target_cameras)
            if len(cams) != O:
                raise L.MvdError(f"generate_views_batch: target_cameras for {len(cams)} objects, prompts for {O}")
            for c in cams:
                if not isinstance(c, torch.Tensor) or c.dim() != 3 or c.shape[0] < 1 or c.shape[1:] != cams[0].shape[1:]:
                    raise L.MvdError("generate_views_batch: a list of target_cameras holds one (V_o, 3|4, 4) tensor per object, V_o >= 1")
            counts = tuple(int(c.shape[0]) for c in cams)
            check_source_cameras(cams[0].shape[1:])
            src = torch.cat([source_cameras[o:o + 1].expand(counts[o], -1, -1) for o in range(O)])
            tgt = torch.cat([c.to(src.device) for c in cams])
            rows, rows_of, layout = sum(counts), f"the {sum(counts)} views of counts {counts}", dict(views=counts)
        else:
            if target_cameras is None or target_cameras.dim() not in (3, 4):
                raise L.MvdError("generate_views_batch: target_cameras must be (O, V, 3|4, 4) or (V, 3|4, 4)")
            tgt = target_cameras if target_cameras.dim() == 4 else target_cameras.unsqueeze(0).expand(O, -1, -1, -1)
            if tgt.shape[0] != O:
                raise L.MvdError(f"generate_views_batch: target_cameras for {tgt.shape[0]} objects, prompts for {O}")
            V = tgt.shape[1]
            check_source_cameras(tgt.shape[2:])
            src, tgt = source_cameras.repeat_interleave(V, 0), tgt.reshape(O * V, *tgt.shape[2:])
            # (one object: generate_views' forward, which is the same function)
            rows, rows_of, layout = O * V, f"{O} objects x {V} views", dict(views=V, objects=None if O == 1 else O)
        return self._turntable(
            prompt_embeds, src, tgt, layout, who="generate_views_batch", rows=rows, rows_of=rows_of,
            sources=O, sources_of=f"one source image per object ({O} rows of source_images or source_image_latents)",
            source_images=source_images, source_image_latents=source_image_latents, height=height, width=width, generator=generator,
            latents=latents, output_type=output_type, return_dict=return_dict, num_inference_steps=num_inference_steps,
            guidance_scale=guidance_scale, negative_prompt_embeds=negative_prompt_embeds, noise_per_step=noise_per_step,
            callback=callback, callback_steps=callback_steps, cross_attention_kwargs=cross_attention_kwargs,
            guidance_rescale=guidance_rescale, **({"apg": apg} if apg is not None else {}))


def _scheduler_from_snapshot(path) -> "Any":
    """DDPM scheduler of the snapshot (``<path>/scheduler/scheduler_config.json``) or SD-2.1's published defaults."""
    from .scheduler import DDPMScheduler
    cfg = {}
    f = os.path.join(str(path), "scheduler", "scheduler_config.json") if path else ""
    if f and os.path.exists(f):
        raw = json.load(open(f))
        cfg = {k: raw[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type",
                                   "timestep_spacing", "steps_offset") if k in raw}
    return DDPMScheduler(**cfg)


SAMPLERS = ("ddpm", "ddim", "dpmsolver++", "unipc")


def _sampler_config_from_snapshot(path) -> Dict[str, Any]:
    """The fields of the snapshot's scheduler config that the DDIM / DPM-Solver++ schedulers read beyond the DDPM ones
    (``steps_offset`` / ``timestep_spacing`` / ``set_alpha_to_one``); {} without a snapshot (the classes' defaults)."""
    f = os.path.join(str(path), "scheduler", "scheduler_config.json") if path else ""
    if not (f and os.path.exists(f)):
        return {}
    raw = json.load(open(f))
    return {k: raw[k] for k in ("steps_offset", "timestep_spacing", "set_alpha_to_one") if k in raw}


def _make_scheduler(path, sampler: str):
    """The interpolated SNR shift (scale 6, mvd_unet.py:420-428) of the snapshot's schedule, handed to the chosen
    sampler's class (``ShiftSNRScheduler.from_scheduler(..., scheduler_class=)``)."""
    from .scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, ShiftSNRScheduler, UniPCMultistepScheduler
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler={sampler!r}: expected one of {SAMPLERS}")
    base_scheduler = _scheduler_from_snapshot(path)
    if sampler == "ddpm":
        return ShiftSNRScheduler.from_scheduler(noise_scheduler=base_scheduler, shift_mode="interpolated", shift_scale=6.0,
                                                scheduler_class=DDPMScheduler)
    base_scheduler.config = SimpleNamespace(**{**vars(base_scheduler.config), **_sampler_config_from_snapshot(path)})
    cls = {"ddim": DDIMScheduler, "dpmsolver++": DPMSolverMultistepScheduler, "unipc": UniPCMultistepScheduler}[sampler]
    return ShiftSNRScheduler.from_scheduler(noise_scheduler=base_scheduler, shift_mode="interpolated", shift_scale=6.0,
                                            scheduler_class=cls)


TEXT_ENCODERS = ("transformers", "hip")


def _native_text_components(path):
    """``CLIPTextModelHIP`` + ``CLIPTokenizerLite`` from the snapshot's ``text_encoder/`` and ``tokenizer/`` (row N5).  Missing
    or unloadable files raise ``MvdError`` -- asking for the native encoder never yields ``None``.  No transformers import."""
    from .clip_tokenizer import CLIPTokenizerLite
    from .text_encoder import CLIPTextModelHIP
    if not path or not os.path.isdir(str(path)):
        raise L.MvdError(f"text_encoder='hip' needs a local snapshot directory with text_encoder/ and tokenizer/ (got {path!r})")
    te_dir, tok_dir = os.path.join(str(path), "text_encoder"), os.path.join(str(path), "tokenizer")
    need = [os.path.join(te_dir, "config.json"), os.path.join(te_dir, "model.safetensors"), os.path.join(tok_dir, "vocab.json"),
            os.path.join(tok_dir, "merges.txt")]
    missing = [f for f in need if not os.path.exists(f)]
    if missing:
        raise L.MvdError(f"text_encoder='hip': snapshot {path} lacks {', '.join(missing)}")
    try:
        tokenizer = CLIPTokenizerLite.from_pretrained(tok_dir)
        text_encoder = CLIPTextModelHIP.from_snapshot(te_dir)
    except L.MvdError:
        raise
    except Exception as e:
        raise L.MvdError(f"text encoder / tokenizer under {path} failed to load: {type(e).__name__}: {e}") from e
    if torch.cuda.is_available():
        text_encoder = text_encoder.to("cuda")
    return text_encoder, tokenizer


def _optional_components(path, dtype, text_encoder_kind: str = "transformers"):
    """VAE / CLIP from a local diffusers snapshot when both the libraries and the files exist; None otherwise.
    ``text_encoder_kind="hip"``: the native encoder and tokenizer instead of transformers' (an error when they cannot load)."""
    vae = text_encoder = tokenizer = None
    if text_encoder_kind == "hip" and (not path or not os.path.isdir(str(path))):
        _native_text_components(path)       # raises
    if not path or not os.path.isdir(str(path)):
        return vae, text_encoder, tokenizer
    try:
        from .vae import AutoencoderKLHIP
    except ImportError:
        AutoencoderKLHIP = None
    if AutoencoderKLHIP is not None and os.path.exists(os.path.join(str(path), "vae", "diffusion_pytorch_model.safetensors")):
        try:
            vae = AutoencoderKLHIP.from_snapshot(os.path.join(str(path), "vae"))
        except Exception as e:   # a snapshot that is there but does not load is an error, not "no VAE"
            raise L.MvdError(f"VAE snapshot under {os.path.join(str(path), 'vae')} failed to load: {type(e).__name__}: {e}") from e
    if text_encoder_kind == "hip":
        text_encoder, tokenizer = _native_text_components(path)
        return vae, text_encoder, tokenizer
    te_dir, tok_dir = os.path.join(str(path), "text_encoder"), os.path.join(str(path), "tokenizer")
    if os.path.isdir(te_dir) and os.path.isdir(tok_dir):
        try:
            from transformers import CLIPTextModel, CLIPTokenizer
        except ImportError:     # no library: the caller passes prompt_embeds (the pipeline says so when asked for a prompt)
            logger.warning("snapshot %s has a text encoder but `transformers` is not importable: pass prompt_embeds", path)
            return vae, None, None
        try:
            tokenizer = CLIPTokenizer.from_pretrained(tok_dir, local_files_only=True)
            text_encoder = CLIPTextModel.from_pretrained(te_dir, local_files_only=True, torch_dtype=dtype)
        except Exception as e:   # files that are there but do not load are an error, not "no text encoder"
            raise L.MvdError(f"text encoder / tokenizer under {path} failed to load: {type(e).__name__}: {e}") from e
    return vae, text_encoder, tokenizer


def build_pipeline(pretrained_model_name_or_path, dtype, use_camera_conditioning, use_image_conditioning, img_ref_scale,
                   cam_modulation_strength, cam_output_dim, cam_hidden_dim, simple_cam_encoder, cache_dir=None,
                   unet_config=None, init: str = "default", *, sampler: str = "ddpm",
                   text_encoder: str = "transformers") -> MVDPipeline:
    """``create_mvd_pipeline`` (mvd_unet.py:388-453): scheduler swap to the interpolated SNR shift (scale 6, hard-coded
    there, :420-428), ``MultiViewUNet`` as ``pipeline.unet``, the three attributes of :449-451.  Nothing is fetched: the
    name resolves to local snapshot files (hub.resolve_snapshot) or the call raises.  ``sampler``: "ddpm" (the
    reference's ancestral DDPM, the default), "ddim", "dpmsolver++" or "unipc" -- the same shifted schedule in another class.
    ``text_encoder``: "transformers" (the default: transformers' CLIP when the package and the snapshot files exist, else none)
    or "hip" (``CLIPTextModelHIP`` + the native tokenizer from the snapshot; an error when they are missing)."""
    from .hub import resolve_snapshot
    from .mvd_unet import MultiViewUNet
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler={sampler!r}: expected one of {SAMPLERS}")
    if text_encoder not in TEXT_ENCODERS:
        raise ValueError(f"text_encoder={text_encoder!r}: expected one of {TEXT_ENCODERS}")
    # MVDPipeline.from_pretrained(name, cache_dir=...) (mvd_unet.py:411-415): a directory, or a hub name whose snapshot is in a
    # local huggingface cache; a name nothing local answers to raises MvdError (never a random-initialised pipeline)
    pretrained_model_name_or_path = resolve_snapshot(pretrained_model_name_or_path, cache_dir)
    scheduler = _make_scheduler(pretrained_model_name_or_path, sampler)
    unet = MultiViewUNet(pretrained_model_name_or_path, dtype=dtype, img_ref_scale=img_ref_scale,
                         cam_modulation_strength=cam_modulation_strength, cam_output_dim=cam_output_dim,
                         cam_hidden_dim=cam_hidden_dim, simple_cam_encoder=simple_cam_encoder,
                         use_camera_conditioning=use_camera_conditioning, use_image_conditioning=use_image_conditioning,
                         unet_config=unet_config, init=init)
    if torch.cuda.is_available():
        unet = unet.to(device="cuda", dtype=dtype)
    vae, text_encoder, tokenizer = _optional_components(pretrained_model_name_or_path, dtype, text_encoder)
    # (StableDiffusionPipeline.__init__: vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1))
    vsf = 2 ** (len(vae.config.block_out_channels) - 1) if vae is not None else 8
    pipe = MVDPipeline(unet, scheduler, vae=vae, text_encoder=text_encoder, tokenizer=tokenizer, vae_scale_factor=vsf)
    pipe.use_camera_conditioning = use_camera_conditioning
    pipe.use_image_conditioning = use_image_conditioning
    pipe.img_ref_scale = img_ref_scale
    return pipe
