"""CLIP image tower and image processor behind the transformers object protocol the reference's validation uses
(val.py:60-196, src/training/losses.py:59-98: ``processor(images=...)["pixel_values"]`` and
``model.get_image_features(pixel_values=...)``), on the HIP kernels of libmvd_hip.so (SURVEY.md 8f row N7,
mvd_amd/csrc/vision.hip).

``CLIPVisionModelHIP`` is an ``nn.Module`` whose parameters carry transformers' state-dict key names of
``CLIPVisionModelWithProjection`` (``vision_model.embeddings.class_embedding`` ... ``vision_model.post_layernorm.bias``,
``visual_projection.weight``), so the vision half of a ``CLIPModel`` file loads with ``load_state_dict`` -- with or without
the leading ``vision_model.``; ``embeddings.position_ids`` is dropped.  It has no torch forward: the calls hand device
pointers to the C ABI (``mvd_vision_preprocess`` / ``mvd_vision_encode``); there is no CPU fallback.  ``transformers`` is
never imported.

Weight slots (``pack_vision``): ``patch.w`` = the patch convolution as ``[H][Kp]`` bf16 rows in ``(c, py, px)`` order, zero
padded from ``3 P^2`` to the next multiple of 64 (the GEMM's K granule: 588 -> 640 at P = 14); ``cls`` ``[H]``, ``pos``
``[tokens][H]``, ``pre_ln`` / ``post_ln`` gains and biases and ``proj.w`` ``[proj][H]`` fp32 (the projection is a GEMV over
one row per image: fp32 weights cost nothing and keep it at fp32 rounding); the layers as in ``pack_text`` (q rows carry
``packing.QSCALE``).
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from .packing import QSCALE, _bf, _f32
from .text_encoder import ACTS, _layer

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_VISION_HEADS = ("embeddings.", "pre_layrnorm.", "encoder.", "post_layernorm.")


class CLIPVisionConfigLite:
    """The fields of transformers' ``CLIPVisionConfig`` the encoder reads (same names, same defaults) + ``projection_dim``."""

    def __init__(self, hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=12, num_attention_heads=12,
                 num_channels=3, image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, **extra):
        self.hidden_size, self.intermediate_size, self.projection_dim = int(hidden_size), int(intermediate_size), int(projection_dim)
        self.num_hidden_layers, self.num_attention_heads, self.num_channels = int(num_hidden_layers), int(num_attention_heads), int(num_channels)
        self.image_size, self.patch_size, self.hidden_act, self.layer_norm_eps = int(image_size), int(patch_size), hidden_act, float(layer_norm_eps)
        for k, v in extra.items():
            setattr(self, k, v)

    @property
    def num_tokens(self) -> int:
        return 1 + (self.image_size // self.patch_size) ** 2

    @property
    def patch_k(self) -> int:
        """Columns of a patch row: 3 P^2 rounded up to the GEMM's K granule of 64."""
        return (3 * self.patch_size ** 2 + 63) // 64 * 64


def normalize_vision_keys(sd):
    """Both key spellings -> ``vision_model.*`` + ``visual_projection.weight``; ``position_ids`` dropped."""
    out = {}
    for k, v in sd.items():
        if k.startswith(_VISION_HEADS):
            k = "vision_model." + k
        if k.endswith("embeddings.position_ids"):
            continue
        out[k] = v
    return out


def split_clip_state_dict(sd):
    """A combined ``CLIPModel`` state dict -> (vision tower incl. ``visual_projection.weight``, text tower with bare keys,
    ``text_projection.weight``); ``logit_scale`` is not used by either score."""
    vision = {k: v for k, v in sd.items() if k.startswith(("vision_model.", "visual_projection."))}
    text = {k[len("text_model."):]: v for k, v in sd.items() if k.startswith("text_model.")}
    if "text_projection.weight" not in sd:
        raise L.MvdError("CLIP state dict has no text_projection.weight")
    return vision, text, sd["text_projection.weight"]


def pack_vision(sd: Dict[str, torch.Tensor], cfg: CLIPVisionConfigLite, device) -> Dict[str, torch.Tensor]:
    """transformers CLIPVisionModelWithProjection state dict (``vision_model.*`` keys) -> the weight slots of vision.hip."""
    out: Dict[str, torch.Tensor] = {}
    f = lambda k: sd[k].detach().float()   # noqa: E731
    v = "vision_model."
    H, K = cfg.hidden_size, 3 * cfg.patch_size ** 2
    pw = torch.zeros(H, cfg.patch_k)
    pw[:, :K] = f(v + "embeddings.patch_embedding.weight").reshape(H, K).cpu()
    out["patch.w"] = _bf(pw, device)
    out["cls"] = _f32(sd[v + "embeddings.class_embedding"], device)
    out["pos"] = _f32(sd[v + "embeddings.position_embedding.weight"], device)
    for src, dst in (("pre_layrnorm", "pre_ln"), ("post_layernorm", "post_ln")):
        out[f"{dst}.g"] = _f32(sd[f"{v}{src}.weight"], device)
        out[f"{dst}.b"] = _f32(sd[f"{v}{src}.bias"], device)
    for i in range(cfg.num_hidden_layers):
        p, s = f"{v}encoder.layers.{i}", f"layers.{i}"
        for src, dst in (("layer_norm1", "ln1"), ("layer_norm2", "ln2")):
            out[f"{s}.{dst}.g"] = _f32(sd[f"{p}.{src}.weight"], device)
            out[f"{s}.{dst}.b"] = _f32(sd[f"{p}.{src}.bias"], device)
        a = f"{p}.self_attn"
        out[f"{s}.qkv.w"] = _bf(torch.cat([f(f"{a}.q_proj.weight") * QSCALE, f(f"{a}.k_proj.weight"), f(f"{a}.v_proj.weight")], 0), device)
        out[f"{s}.qkv.b"] = _f32(torch.cat([f(f"{a}.q_proj.bias") * QSCALE, f(f"{a}.k_proj.bias"), f(f"{a}.v_proj.bias")], 0), device)
        for src, dst in ((f"{a}.out_proj", "out"), (f"{p}.mlp.fc1", "fc1"), (f"{p}.mlp.fc2", "fc2")):
            out[f"{s}.{dst}.w"] = _bf(sd[f"{src}.weight"], device)
            out[f"{s}.{dst}.b"] = _f32(sd[f"{src}.bias"], device)
    out["proj.w"] = _f32(sd["visual_projection.weight"], device)
    return out


def _f3(values):
    return (C.c_float * 3)(*[float(x) for x in values])


class _VisionHandle(L.Handle):
    """One ``mvd_vision_t`` with its workspace and the resize geometry the resampling tables at its head belong to."""

    def __init__(self, cfg: CLIPVisionConfigLite):
        c = L.mvd_vision_config_t()
        c.image_size, c.patch_size, c.hidden_size, c.intermediate_size = cfg.image_size, cfg.patch_size, cfg.hidden_size, cfg.intermediate_size
        c.num_layers, c.num_heads, c.projection_dim = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.projection_dim
        c.layer_norm_eps, c.act = cfg.layer_norm_eps, ACTS[cfg.hidden_act]
        super().__init__("vision", C.byref(c))
        self.geometry = (0, 0, 0)

    def workspace(self, device, batch, h=0, w=0, resize_to=0):
        if h == 0:                     # encode only: the resampling tables of the last geometry stay where they are
            h, w, resize_to = self.geometry
        self.geometry = (h, w, resize_to)
        super().workspace(device, batch, h, w, resize_to)

    def preprocess(self, images, quantize, resize_to, crop, mean, std, want_patches, want_pixel_values):
        B, ch, h, w = images.shape
        if ch != 3:
            raise L.MvdError(f"CLIP preprocessing takes 3-channel images, got {tuple(images.shape)}")
        self.workspace(images.device, B, h, w, resize_to)
        pv = torch.empty(B, 3, crop, crop, device=images.device, dtype=torch.float32) if want_pixel_values else None
        L.call("mvd_vision_preprocess", self.h, C.c_void_p(images.data_ptr()), B, h, w, int(quantize), int(resize_to), int(crop),
               _f3(mean), _f3(std), int(want_patches), C.c_void_p(pv.data_ptr()) if pv is not None else None, L.stream())
        return pv


def _device_images(images, who) -> torch.Tensor:
    """(B, 3, H, W) fp32 contiguous on the GPU from a tensor / a list of equally sized (3, H, W) tensors."""
    if isinstance(images, (list, tuple)):
        if not images or len({tuple(i.shape) for i in images}) != 1:
            raise L.MvdError(f"{who}: a list of images must be non-empty and of one size (one resize geometry per call)")
        images = torch.stack(list(images))
    if not isinstance(images, torch.Tensor):
        raise L.MvdError(f"{who}: images must be torch tensors (C, H, W) / (B, C, H, W), got {type(images).__name__}")
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[0] < 1:
        raise L.MvdError(f"{who}: images must be (B, 3, H, W), got {tuple(images.shape)}")
    if not images.is_cuda:
        if not torch.cuda.is_available():
            raise L.MvdError(f"{who} needs a MI355X (there is no CPU fallback)")
        images = images.cuda()
    return images.to(torch.float32).contiguous()


class BatchFeatureLite(dict):
    """What ``processor(...)`` returns: a mapping with ``["pixel_values"]`` and ``.to(device)``."""

    def to(self, *args, **kwargs):
        return BatchFeatureLite({k: v.to(*args, **kwargs) for k, v in self.items()})

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class CLIPImageProcessorLite:
    """``CLIPImageProcessor`` for uint8 image tensors, on the device: shortest-edge BICUBIC resize (PIL's 8-bit arithmetic,
    byte for byte), centre crop, 1 / 255, normalisation -- ``mvd_vision_preprocess``.  Only that pipeline is implemented: a
    config that switches a step off, asks for another filter or another rescale factor is an error, never an approximation."""

    def __init__(self, size=224, crop_size=224, image_mean: Sequence[float] = OPENAI_CLIP_MEAN, image_std: Sequence[float] = OPENAI_CLIP_STD,
                 resample: int = 3, do_resize=True, do_center_crop=True, do_rescale=True, do_normalize=True, rescale_factor=1 / 255,
                 **_ignored):
        if isinstance(size, dict):
            if "shortest_edge" not in size:
                raise L.MvdError(f"CLIPImageProcessorLite: size={size!r}: only the shortest-edge rule is implemented")
            size = size["shortest_edge"]
        if isinstance(crop_size, dict):
            if crop_size.get("height") != crop_size.get("width"):
                raise L.MvdError(f"CLIPImageProcessorLite: crop_size={crop_size!r}: only square crops are implemented")
            crop_size = crop_size["height"]
        if int(resample) != 3:
            raise L.MvdError(f"CLIPImageProcessorLite: resample={resample!r}: only PIL's BICUBIC (3) is implemented")
        if not (do_resize and do_center_crop and do_rescale and do_normalize):
            raise L.MvdError("CLIPImageProcessorLite: do_resize, do_center_crop, do_rescale and do_normalize must all be on")
        if abs(float(rescale_factor) - 1 / 255) > 1e-12:
            raise L.MvdError(f"CLIPImageProcessorLite: rescale_factor={rescale_factor!r}: only 1/255 is implemented")
        self.size, self.crop_size = int(size), int(crop_size)
        if self.size < self.crop_size:
            raise L.MvdError(f"CLIPImageProcessorLite: size {self.size} < crop_size {self.crop_size} would need padding (not implemented)")
        self.image_mean, self.image_std = tuple(float(x) for x in image_mean), tuple(float(x) for x in image_std)
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise L.MvdError("CLIPImageProcessorLite: image_mean / image_std must have three entries")
        self._handle = None

    @classmethod
    def from_pretrained(cls, path: str, **_ignored) -> "CLIPImageProcessorLite":
        """``<path>/preprocessor_config.json`` of a local directory (nothing is fetched)."""
        with open(os.path.join(path, "preprocessor_config.json"), encoding="utf-8") as f:
            raw = json.load(f)
        keys = ("size", "crop_size", "image_mean", "image_std", "resample", "do_resize", "do_center_crop", "do_rescale", "do_normalize",
                "rescale_factor")
        return cls(**{k: raw[k] for k in keys if raw.get(k) is not None})

    def __call__(self, images=None, return_tensors="pt", padding=None, **_ignored) -> BatchFeatureLite:
        if return_tensors not in ("pt", None):
            raise L.MvdError(f"CLIPImageProcessorLite: return_tensors={return_tensors!r} (only 'pt')")
        x = _device_images(images, "CLIPImageProcessorLite")
        if self._handle is None:       # preprocessing needs no model: the smallest handle the ABI makes
            self._handle = _VisionHandle(CLIPVisionConfigLite(hidden_size=64, intermediate_size=64, projection_dim=64, num_hidden_layers=0,
                                                              num_attention_heads=1, image_size=1, patch_size=1))
        pv = self._handle.preprocess(x, False, self.size, self.crop_size, self.image_mean, self.image_std, False, True)
        return BatchFeatureLite(pixel_values=pv)


class VisionEncoderOutput(tuple):
    """``out[0]`` / ``.last_hidden_state`` (B, tokens, hidden); ``out[1]`` / ``.image_embeds`` (B, projection_dim); fp32, on the device."""

    @property
    def last_hidden_state(self):
        return self[0]

    @property
    def image_embeds(self):
        return self[1]


class CLIPVisionModelHIP(nn.Module):
    def __init__(self, config: Optional[CLIPVisionConfigLite] = None):
        super().__init__()
        self.config = cfg = config or CLIPVisionConfigLite()
        if cfg.hidden_act not in ACTS:
            raise L.MvdError(f"CLIPVisionModelHIP: hidden_act={cfg.hidden_act!r}: expected one of {tuple(ACTS)}")
        if cfg.num_attention_heads <= 0 or cfg.hidden_size != 64 * cfg.num_attention_heads:
            raise L.MvdError(f"CLIPVisionModelHIP: hidden_size {cfg.hidden_size} / num_attention_heads {cfg.num_attention_heads}: "
                             "the attention kernel takes a head dimension of 64")
        if cfg.patch_size <= 0 or cfg.image_size <= 0 or cfg.image_size % cfg.patch_size:
            raise L.MvdError(f"CLIPVisionModelHIP: image_size {cfg.image_size} must be a multiple of patch_size {cfg.patch_size}")
        if cfg.hidden_size > 2048 or cfg.intermediate_size % 64 or cfg.projection_dim % 64 or not 0 < cfg.projection_dim <= 2048 or cfg.num_channels != 3:
            raise L.MvdError("CLIPVisionModelHIP: hidden_size <= 2048, intermediate_size % 64 == 0, projection_dim % 64 == 0 (<= 2048) and "
                             f"3 channels are required (got {cfg.hidden_size}, {cfg.intermediate_size}, {cfg.projection_dim}, {cfg.num_channels})")
        h = cfg.hidden_size
        vm = nn.Module()
        vm.embeddings = nn.Module()
        vm.embeddings.class_embedding = nn.Parameter(torch.randn(h))
        vm.embeddings.patch_embedding = nn.Conv2d(3, h, cfg.patch_size, cfg.patch_size, bias=False)
        vm.embeddings.position_embedding = nn.Embedding(cfg.num_tokens, h)
        vm.pre_layrnorm = nn.LayerNorm(h)
        vm.encoder = nn.Module()
        vm.encoder.layers = nn.ModuleList([_layer(h, cfg.intermediate_size) for _ in range(cfg.num_hidden_layers)])
        vm.post_layernorm = nn.LayerNorm(h)
        self.vision_model = vm
        self.visual_projection = nn.Linear(h, cfg.projection_dim, bias=False)
        self._handle = None
        self._dev = None
        self._packed: Dict[str, torch.Tensor] = {}
        self._dirty = True

    def load_state_dict(self, sd, strict: bool = True, **kw):
        self._dirty = True
        return super().load_state_dict(normalize_vision_keys(sd), strict=strict, **kw)

    def to(self, *a, **k):
        self._dirty = True
        return super().to(*a, **k)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container; the arithmetic runs in libmvd_hip.so")

    # ------------------------------------------------------------------ engine plumbing
    def _sync(self) -> torch.device:
        if not torch.cuda.is_available():
            raise L.MvdError("CLIPVisionModelHIP needs a MI355X (there is no CPU fallback)")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.MvdError(f"CLIPVisionModelHIP is on {dev}: move it to a cuda device (there is no CPU fallback)")
        if self._handle is None:
            self._handle = _VisionHandle(self.config)
        if self._dirty or self._dev != dev:
            with torch.no_grad():
                self._packed = pack_vision(self.state_dict(), self.config, dev)
            self._handle.set_weights(self._packed)
            self._dirty, self._dev = False, dev
        return dev

    def _encode(self, pixel_values, batch, want_hidden=False):
        cfg, dev = self.config, self._dev
        hid = torch.empty(batch, cfg.num_tokens, cfg.hidden_size, device=dev, dtype=torch.float32) if want_hidden else None
        raw = torch.empty(batch, cfg.projection_dim, device=dev, dtype=torch.float32)
        nrm = torch.empty_like(raw)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        L.call("mvd_vision_encode", self._handle.h, p(pixel_values), batch, p(hid), p(raw), p(nrm), L.stream())
        return hid, raw, nrm

    def _check_pixel_values(self, pixel_values):
        s = self.config.image_size
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, s, s) or pixel_values.shape[0] < 1:
            raise L.MvdError(f"CLIPVisionModelHIP: pixel_values must be (B, 3, {s}, {s}), got {tuple(getattr(pixel_values, 'shape', ()))}")
        return pixel_values.to(self._sync(), torch.float32).contiguous()

    # ------------------------------------------------------------------ the transformers protocol
    @torch.no_grad()
    def encode(self, pixel_values: torch.Tensor, want_hidden: bool = False):
        """-> (last_hidden_state or None, image_embeds, L2-normalised image_embeds)."""
        pv = self._check_pixel_values(pixel_values)
        self._handle.workspace(pv.device, pv.shape[0])
        return self._encode(pv, pv.shape[0], want_hidden)

    def get_image_features(self, pixel_values: torch.Tensor = None, **_ignored) -> torch.Tensor:
        return self.encode(pixel_values)[1]

    def __call__(self, pixel_values: torch.Tensor = None, **_ignored) -> VisionEncoderOutput:
        hid, raw, _ = self.encode(pixel_values, want_hidden=True)
        return VisionEncoderOutput((hid, raw))

    # ------------------------------------------------------------------ the fused route
    @torch.no_grad()
    def embed_images(self, images, processor: CLIPImageProcessorLite, quantize: bool):
        """Images straight to embeddings: fp32 (B, 3, H, W) in [-1, 1] (``quantize``) or uint8-valued -> preprocessing writes the
        bf16 patch rows into the workspace, the encoder reads them there.  -> (image_embeds, normalised); nothing synchronises."""
        dev = self._sync()
        x = _device_images(images, "CLIPVisionModelHIP").to(dev)
        if processor.crop_size != self.config.image_size:
            raise L.MvdError(f"CLIPVisionModelHIP: the processor crops to {processor.crop_size}, the model takes {self.config.image_size}")
        self._handle.preprocess(x, quantize, processor.size, processor.crop_size, processor.image_mean, processor.image_std, True, False)
        _, raw, nrm = self._encode(None, x.shape[0])
        return raw, nrm
