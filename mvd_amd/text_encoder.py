"""CLIP text encoder behind the transformers object protocol the reference pipeline uses
(/root/reference/src/models/pipeline.py:52-75 ``text_encoder(input_ids)[0]``), on the HIP kernels of libmvd_hip.so
(mvd_amd/csrc/text.hip).

``CLIPTextModelHIP`` is an ``nn.Module`` whose parameters carry transformers' state-dict key names
(``embeddings.token_embedding.weight`` ... ``final_layer_norm.bias``), so ``text_encoder/model.safetensors`` of a local
snapshot loads with ``load_state_dict`` -- with or without the leading ``text_model.`` (published SD-2.1 files carry it,
recent transformers releases write ``state_dict()`` without it); ``embeddings.position_ids`` is dropped.  It has no torch
forward: ``__call__`` hands device pointers to the C ABI (``mvd_text_encode``); there is no CPU fallback.  ``transformers``
is never imported.

Weight slots (``pack_text``): ``tok`` / ``pos`` embedding tables fp32 (a gather reads 77 rows per prompt, so their width
costs no time, and they start the fp32 residual stream unrounded); per layer ``layers.N.qkv.w`` = [q; k; v] rows
concatenated ``[3H][H]`` bf16 with the q rows (and ``qkv.b``'s q part) carrying ``64^-0.5 * log2(e)`` (``packing.QSCALE``),
``out.w`` ``[H][H]``, ``fc1.w`` ``[I][H]``, ``fc2.w`` ``[H][I]`` bf16; LayerNorm gains / biases and linear biases fp32.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .packing import QSCALE, _bf, _f32

ACTS = {"gelu": 0, "quick_gelu": 1}


class CLIPTextConfigLite:
    """The fields of transformers' ``CLIPTextConfig`` the encoder reads (same names, same defaults)."""

    def __init__(self, vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                 max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, **extra):
        self.vocab_size, self.hidden_size, self.intermediate_size = int(vocab_size), int(hidden_size), int(intermediate_size)
        self.num_hidden_layers, self.num_attention_heads = int(num_hidden_layers), int(num_attention_heads)
        self.max_position_embeddings, self.hidden_act, self.layer_norm_eps = int(max_position_embeddings), hidden_act, float(layer_norm_eps)
        for k, v in extra.items():
            setattr(self, k, v)


def _layer(h, i):
    m = nn.Module()
    m.layer_norm1, m.layer_norm2 = nn.LayerNorm(h), nn.LayerNorm(h)
    a = nn.Module()
    a.q_proj, a.k_proj, a.v_proj, a.out_proj = nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h)
    m.self_attn = a
    f = nn.Module()
    f.fc1, f.fc2 = nn.Linear(h, i), nn.Linear(i, h)
    m.mlp = f
    return m


def strip_text_model_prefix(sd):
    """Both key spellings -> the bare one; ``position_ids`` (a buffer of older transformers releases) dropped."""
    out = {}
    for k, v in sd.items():
        if k.startswith("text_model."):
            k = k[len("text_model."):]
        if k.endswith("embeddings.position_ids"):
            continue
        out[k] = v
    return out


def pack_text(sd: Dict[str, torch.Tensor], cfg: CLIPTextConfigLite, device) -> Dict[str, torch.Tensor]:
    """transformers CLIPTextModel state dict (bare keys) -> the engine's weight slots (mvd_amd/csrc/text.hip)."""
    out: Dict[str, torch.Tensor] = {}
    f = lambda k: sd[k].detach().float()   # noqa: E731
    out["tok"] = _f32(sd["embeddings.token_embedding.weight"], device)
    out["pos"] = _f32(sd["embeddings.position_embedding.weight"], device)
    for i in range(cfg.num_hidden_layers):
        p, s = f"encoder.layers.{i}", f"layers.{i}"
        for src, dst in (("layer_norm1", "ln1"), ("layer_norm2", "ln2")):
            out[f"{s}.{dst}.g"] = _f32(sd[f"{p}.{src}.weight"], device)
            out[f"{s}.{dst}.b"] = _f32(sd[f"{p}.{src}.bias"], device)
        a = f"{p}.self_attn"
        out[f"{s}.qkv.w"] = _bf(torch.cat([f(f"{a}.q_proj.weight") * QSCALE, f(f"{a}.k_proj.weight"), f(f"{a}.v_proj.weight")], 0), device)
        out[f"{s}.qkv.b"] = _f32(torch.cat([f(f"{a}.q_proj.bias") * QSCALE, f(f"{a}.k_proj.bias"), f(f"{a}.v_proj.bias")], 0), device)
        for src, dst in ((f"{a}.out_proj", "out"), (f"{p}.mlp.fc1", "fc1"), (f"{p}.mlp.fc2", "fc2")):
            out[f"{s}.{dst}.w"] = _bf(sd[f"{src}.weight"], device)
            out[f"{s}.{dst}.b"] = _f32(sd[f"{src}.bias"], device)
    out["final_ln.g"] = _f32(sd["final_layer_norm.weight"], device)
    out["final_ln.b"] = _f32(sd["final_layer_norm.bias"], device)
    return out


class TextEncoderOutput(tuple):
    """``out[0]`` / ``out.last_hidden_state``: (B, T, hidden) fp32 on the device."""

    @property
    def last_hidden_state(self):
        return self[0]


class CLIPTextModelHIP(nn.Module):
    def __init__(self, config: Optional[CLIPTextConfigLite] = None):
        super().__init__()
        self.config = cfg = config or CLIPTextConfigLite()
        if cfg.hidden_act not in ACTS:
            raise L.MvdError(f"CLIPTextModelHIP: hidden_act={cfg.hidden_act!r}: expected one of {tuple(ACTS)}")
        if cfg.num_attention_heads <= 0 or cfg.hidden_size != 64 * cfg.num_attention_heads:
            raise L.MvdError(f"CLIPTextModelHIP: hidden_size {cfg.hidden_size} / num_attention_heads {cfg.num_attention_heads}: "
                             "the attention kernel takes a head dimension of 64")
        if cfg.hidden_size > 2048 or cfg.intermediate_size % 64 or not 0 < cfg.max_position_embeddings <= 96:
            raise L.MvdError("CLIPTextModelHIP: hidden_size <= 2048, intermediate_size % 64 == 0 and max_position_embeddings <= 96 "
                             f"are required (got {cfg.hidden_size}, {cfg.intermediate_size}, {cfg.max_position_embeddings})")
        h = cfg.hidden_size
        self.embeddings = nn.Module()
        self.embeddings.token_embedding = nn.Embedding(cfg.vocab_size, h)
        self.embeddings.position_embedding = nn.Embedding(cfg.max_position_embeddings, h)
        self.encoder = nn.Module()
        self.encoder.layers = nn.ModuleList([_layer(h, cfg.intermediate_size) for _ in range(cfg.num_hidden_layers)])
        self.final_layer_norm = nn.LayerNorm(h)
        self._handle: Optional[L.Handle] = None
        self._dev = None
        self._packed: Dict[str, torch.Tensor] = {}
        self._dirty = True

    @property
    def _h(self):
        return self._handle.h if self._handle is not None else None

    @property
    def _ws(self):
        return self._handle.ws if self._handle is not None else None

    @classmethod
    def from_snapshot(cls, path: str) -> "CLIPTextModelHIP":
        """``<path>/config.json`` + ``model.safetensors`` of a local snapshot's ``text_encoder`` directory (nothing is fetched)."""
        raw = json.load(open(os.path.join(path, "config.json")))
        keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                "max_position_embeddings", "hidden_act", "layer_norm_eps")
        m = cls(CLIPTextConfigLite(**{k: raw[k] for k in keys if k in raw}))
        from safetensors.torch import load_file
        m.load_state_dict(load_file(os.path.join(path, "model.safetensors")))
        return m

    def load_state_dict(self, sd, strict: bool = True, **kw):
        self._dirty = True
        return super().load_state_dict(strip_text_model_prefix(sd), strict=strict, **kw)

    def to(self, *a, **k):
        self._dirty = True
        return super().to(*a, **k)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container; the arithmetic runs in libmvd_hip.so")

    # ------------------------------------------------------------------ engine plumbing
    def _sync(self) -> torch.device:
        if not torch.cuda.is_available():
            raise L.MvdError("CLIPTextModelHIP needs a MI355X (there is no CPU fallback)")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.MvdError(f"CLIPTextModelHIP is on {dev}: move it to a cuda device (there is no CPU fallback)")
        if self._handle is None:
            c, cfg = L.mvd_text_config_t(), self.config
            c.vocab_size, c.hidden_size, c.intermediate_size = cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size
            c.num_layers, c.num_heads, c.max_positions = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.max_position_embeddings
            c.layer_norm_eps, c.act = cfg.layer_norm_eps, ACTS[cfg.hidden_act]
            self._handle = L.Handle("text", C.byref(c), rebind_always=True)
        if self._dirty or self._dev != dev:
            with torch.no_grad():
                self._packed = pack_text(self.state_dict(), self.config, dev)
            self._handle.set_weights(self._packed)
            self._dirty, self._dev = False, dev
        return dev

    # ------------------------------------------------------------------ the transformers protocol
    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, **_ignored) -> TextEncoderOutput:
        if input_ids.dim() != 2:
            raise L.MvdError(f"CLIPTextModelHIP: input_ids must be (batch, seq_len), got {tuple(input_ids.shape)}")
        B, T = input_ids.shape
        if T > self.config.max_position_embeddings or B < 1 or T < 1:
            raise L.MvdError(f"CLIPTextModelHIP: seq_len {T} (batch {B}) exceeds max_position_embeddings {self.config.max_position_embeddings}")
        # one reduction per call, outside the denoising loop: the kernel clamps ids for address safety only
        lo, hi = (int(v) for v in torch.aminmax(input_ids))
        if lo < 0 or hi >= self.config.vocab_size:
            raise L.MvdError(f"CLIPTextModelHIP: token ids must be in [0, {self.config.vocab_size}), got [{lo}, {hi}]")
        dev = self._sync()
        ids = input_ids.to(dev, torch.int32).contiguous()
        self._handle.workspace(dev, B, T)
        out = torch.empty(B, T, self.config.hidden_size, device=dev, dtype=torch.float32)
        L.call("mvd_text_encode", self._h, C.c_void_p(ids.data_ptr()), B, T, C.c_void_p(out.data_ptr()), L.stream())
        return TextEncoderOutput((out,))
