"""CLIP score for checkpoint validation on this project's kernels: the object the reference builds
as ``torchmetrics.multimodal.CLIPScore(model_name_or_path=...)`` (val.py:60-196) and hands to
``compute_losses`` as ``clip_score_metric_obj`` (src/training/losses.py:59-98, 263), without torchmetrics, transformers,
torchvision or PIL.

``CLIPScore(name_or_path, cache_dir=None)`` resolves a local snapshot of a CLIP model (``hub.resolve_snapshot``: nothing is
fetched) holding ``config.json`` (``text_config`` / ``vision_config`` / ``projection_dim``), ``model.safetensors`` (the
combined ``CLIPModel`` state dict), ``preprocessor_config.json``, ``vocab.json`` and ``merges.txt``; a missing or unloadable
file raises ``MvdError``.  It offers what both reference call sites use:

* ``.to(device)``, ``.processor(images=uint8, return_tensors="pt", padding=True)``, ``.model.get_image_features(pixel_values=)``,
  ``.model.get_text_features(input_ids=, attention_mask=None)`` -- so ``_calculate_clip_score`` runs on it unchanged;
* ``metric(images_uint8, prompts)`` / ``update`` / ``compute`` / ``reset`` with torchmetrics' arithmetic (1.6: per-sample
  ``100 cos``, ``update`` adds the sum and the count, ``compute`` = ``max(sum / n, 0)`` -- the clamp is on the mean);
* ``image_similarity(a, b)``: the fused route for two [-1, 1] image batches -- preprocess, encode, cosine -- a 0-d device
  tensor, no host synchronisation.

One difference from torchmetrics is deliberate: a prompt longer than the context is truncated by the tokenizer (77 tokens WITH
the end token), where torchmetrics 1.6 slices the ids to 77 and drops it.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Sequence, Union

import torch

from . import _lib as L
from .clip_tokenizer import CLIPTokenizerLite
from .hub import resolve_snapshot
from .text_encoder import CLIPTextConfigLite, CLIPTextModelHIP
from .vision_encoder import CLIPImageProcessorLite, CLIPVisionConfigLite, CLIPVisionModelHIP, split_clip_state_dict

FILES = ("config.json", "model.safetensors", "preprocessor_config.json", "vocab.json", "merges.txt")
_TEXT_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
              "hidden_act", "layer_norm_eps")
_VISION_KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_channels", "image_size", "patch_size",
                "hidden_act", "layer_norm_eps")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def clip_cosine(a: torch.Tensor, b: torch.Tensor):
    """(per-row dot products, their mean as a 0-d tensor) of two (B, D) fp32 arrays of L2-normalised rows (``mvd_op_clip_cosine``)."""
    if a.shape != b.shape or a.dim() != 2 or not a.is_cuda:
        raise L.MvdError(f"clip_cosine: two equal (B, D) CUDA arrays expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = a.float().contiguous(), b.float().contiguous()
    rows = torch.empty(a.shape[0], device=a.device, dtype=torch.float32)
    mean = torch.empty((), device=a.device, dtype=torch.float32)
    L.call("mvd_op_clip_cosine", _p(a), _p(b), a.shape[0], a.shape[1], _p(rows), _p(mean), L.stream())
    return rows, mean


def pool_project(hidden: torch.Tensor, proj_w: torch.Tensor, ids=None, eos_token_id: int = 2, delta=None, ln=None, eps: float = 1e-5):
    """``mvd_op_clip_pool_project``: hidden (B, T, H) fp32, proj_w (P, H) fp32 -> (embeds, L2-normalised embeds), (B, P) fp32.
    ``ids`` (B, T): the text tower's pooled position (see include/mvd_hip.h); None: token 0.  ``ln``: (gain, bias) or None."""
    B, T, H = hidden.shape
    hidden, proj_w = hidden.float().contiguous(), proj_w.float().contiguous()
    ids32 = ids.to(hidden.device, torch.int32).contiguous() if ids is not None else None
    delta = delta.float().contiguous() if delta is not None else None
    g, b = (ln[0].float().contiguous(), ln[1].float().contiguous()) if ln is not None else (None, None)
    raw = torch.empty(B, proj_w.shape[0], device=hidden.device, dtype=torch.float32)
    nrm = torch.empty_like(raw)
    L.call("mvd_op_clip_pool_project", _p(hidden), _p(delta), _p(ids32), B, T, H, int(eos_token_id), _p(g), _p(b), float(eps), _p(proj_w),
           proj_w.shape[0], _p(raw), _p(nrm), L.stream())
    return raw, nrm


class CLIPModelHIP:
    """The two towers behind ``get_image_features`` / ``get_text_features`` of transformers' ``CLIPModel``."""

    def __init__(self, vision: CLIPVisionModelHIP, text: CLIPTextModelHIP, text_projection: torch.Tensor, eos_token_id: int):
        self.vision_model_hip, self.text_model_hip = vision, text
        self.text_projection = text_projection.detach().float().contiguous()
        self.eos_token_id = int(eos_token_id)
        if self.text_projection.shape != (vision.config.projection_dim, text.config.hidden_size):
            raise L.MvdError(f"CLIPModelHIP: text_projection.weight is {tuple(self.text_projection.shape)}, expected "
                             f"({vision.config.projection_dim}, {text.config.hidden_size})")

    def to(self, device=None, *_a, **_k):
        if device is not None and torch.device(device) != self.text_projection.device:
            self.vision_model_hip.to(device)
            self.text_model_hip.to(device)
            self.text_projection = self.text_projection.to(device)
        return self

    def eval(self):
        return self

    @property
    def device(self):
        return self.text_projection.device

    def get_image_features(self, pixel_values=None, **_ignored) -> torch.Tensor:
        return self.vision_model_hip.get_image_features(pixel_values=pixel_values)

    @torch.no_grad()
    def text_features(self, input_ids: torch.Tensor):
        """-> (text_embeds, L2-normalised).  No attention mask: with a causal tower the pooled end-token row does not depend on
        the padding behind it (tests/test_text_encoder_gpu.py::test_encoder_causality_is_exact)."""
        hidden = self.text_model_hip(input_ids)[0]
        return pool_project(hidden, self.text_projection.to(hidden.device), ids=input_ids, eos_token_id=self.eos_token_id)

    def get_text_features(self, input_ids=None, attention_mask=None, **_ignored) -> torch.Tensor:
        return self.text_features(input_ids)[0]


class CLIPScore:
    def __init__(self, model_name_or_path: str, cache_dir=None, **_ignored):
        snap = resolve_snapshot(model_name_or_path, cache_dir=cache_dir)
        for name in FILES:
            if not os.path.isfile(os.path.join(snap, name)):
                raise L.MvdError(f"CLIPScore: the snapshot {snap} lacks {name} (needed: {', '.join(FILES)}); nothing is fetched")
        try:
            with open(os.path.join(snap, "config.json"), encoding="utf-8") as f:
                raw = json.load(f)
            tc, vc = raw.get("text_config") or {}, raw.get("vision_config") or {}
            proj = int(raw.get("projection_dim", tc.get("projection_dim", vc.get("projection_dim", 512))))
            text_cfg = CLIPTextConfigLite(**{k: tc[k] for k in _TEXT_KEYS if k in tc})
            vision_cfg = CLIPVisionConfigLite(projection_dim=proj, **{k: vc[k] for k in _VISION_KEYS if k in vc})
            eos = int(tc.get("eos_token_id", 49407))
            from safetensors.torch import load_file
            vsd, tsd, tproj = split_clip_state_dict(load_file(os.path.join(snap, "model.safetensors")))
            vision, text = CLIPVisionModelHIP(vision_cfg), CLIPTextModelHIP(text_cfg)
            vision.load_state_dict(vsd)
            text.load_state_dict(tsd)
            self.model = CLIPModelHIP(vision, text, tproj, eos)
            self.processor = CLIPImageProcessorLite.from_pretrained(snap)
            self.tokenizer = CLIPTokenizerLite.from_pretrained(snap)
        except L.MvdError:
            raise
        except Exception as e:      # a truncated file, a key of the wrong shape, a config that is not JSON: one error type
            raise L.MvdError(f"CLIPScore: the snapshot {snap} could not be loaded: {type(e).__name__}: {e}") from e
        if self.processor.crop_size != vision_cfg.image_size:
            raise L.MvdError(f"CLIPScore: preprocessor crop_size {self.processor.crop_size} != vision image_size {vision_cfg.image_size}")
        self.max_length = min(self.tokenizer.model_max_length, text_cfg.max_position_embeddings)
        self._sum = None
        self._n = 0

    # ------------------------------------------------------------------ placement
    def to(self, device=None, *_a, **_k):
        self.model.to(device)
        return self

    @property
    def device(self):
        return self.model.device

    def _cuda(self):
        if self.device.type != "cuda":
            if not torch.cuda.is_available():
                raise L.MvdError("CLIPScore needs a MI355X (there is no CPU fallback)")
            self.to(torch.device("cuda", torch.cuda.current_device()))
        return self.device

    # ------------------------------------------------------------------ torchmetrics' protocol
    def _ids(self, prompts: Union[str, Sequence[str]]) -> torch.Tensor:
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        return self.tokenizer(prompts, padding=True, truncation=True, max_length=self.max_length, return_tensors="pt").input_ids

    @torch.no_grad()
    def scores(self, images, prompts) -> torch.Tensor:
        """Per-sample ``100 cos(image, prompt)``, (B,) on the device."""
        dev = self._cuda()
        ids = self._ids(prompts).to(dev)
        _, img = self.model.vision_model_hip.embed_images(images, self.processor, quantize=False)
        if img.shape[0] != ids.shape[0]:
            raise ValueError(f"CLIPScore: {img.shape[0]} images but {ids.shape[0]} prompts")
        _, txt = self.model.text_features(ids)
        return 100.0 * clip_cosine(img, txt)[0]

    def update(self, images, text) -> None:
        s = self.scores(images, text)
        total = s.sum()
        self._sum = total if self._sum is None else self._sum + total
        self._n += s.numel()

    def compute(self) -> torch.Tensor:
        if self._sum is None:
            raise L.MvdError("CLIPScore.compute() before any update()")
        return torch.clamp(self._sum / self._n, min=0.0)

    def reset(self) -> None:
        self._sum, self._n = None, 0

    def __call__(self, images, text) -> torch.Tensor:
        """torchmetrics' ``forward``: the score of this batch (clamped mean), which also enters the running state."""
        s = self.scores(images, text)
        total = s.sum()
        self._sum = total if self._sum is None else self._sum + total
        self._n += s.numel()
        return torch.clamp(total / s.numel(), min=0.0)

    forward = __call__

    # ------------------------------------------------------------------ the fused image-to-image route
    @torch.no_grad()
    def image_similarity(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """losses.py:59-98 in three stages per batch and one cosine: a, b (B, 3, H, W) in [-1, 1] -> the mean cosine of their
        CLIP image embeddings, a 0-d device tensor.  The uint8 quantisation of losses.py:11-13 is the first step of the
        preprocessing kernel."""
        self._cuda()
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"image_similarity: batches of {a.shape[0]} and {b.shape[0]} images")
        vis = self.model.vision_model_hip
        _, na = vis.embed_images(a, self.processor, quantize=True)
        _, nb = vis.embed_images(b, self.processor, quantize=True)
        return clip_cosine(na, nb)[1]
