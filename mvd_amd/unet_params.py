"""Parameter containers mirroring diffusers' ``UNet2DConditionModel`` module tree (SD-2.x layout).

These modules exist to own parameters under the exact diffusers state-dict key names
(so Lightning checkpoints of the reference load with ``load_state_dict``), to expose the
attributes the reference pokes at (``attn.to_q.in_features``, ``attn.heads``,
``attn.processor``, ``block.attentions[j].transformer_blocks``) and nothing else: they have
NO torch forward -- the arithmetic lives in libmvd_hip.so.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch.nn as nn

from .attention import AttnProcessor2_0HIP
from .config import UNetConfig


class _NoForward(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(f"{type(self).__name__} is a parameter container; the forward runs in the MVD HIP engine")



class Attention(_NoForward):
    def __init__(self, query_dim, cross_dim, heads, dim_head=64):
        super().__init__()
        inner = heads * dim_head
        self.heads = heads
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(cross_dim, inner, bias=False)
        self.to_v = nn.Linear(cross_dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(0.0)])
        self.processor = AttnProcessor2_0HIP()     # diffusers' default processor, on the HIP kernels


class GEGLU(_NoForward):
    def __init__(self, dim, inner):
        super().__init__()
        self.proj = nn.Linear(dim, inner * 2)


class FeedForward(_NoForward):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, 4 * dim), nn.Dropout(0.0), nn.Linear(4 * dim, dim)])


class BasicTransformerBlock(_NoForward):
    def __init__(self, dim, heads, cross_dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, dim, heads)
        self.norm2 = nn.LayerNorm(dim)
        self.attn2 = Attention(dim, cross_dim, heads)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim)


class Transformer2DModel(_NoForward):
    def __init__(self, dim, heads, cross_dim, groups):
        super().__init__()
        self.norm = nn.GroupNorm(groups, dim, eps=1e-6)
        self.proj_in = nn.Linear(dim, dim)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(dim, heads, cross_dim)])
        self.proj_out = nn.Linear(dim, dim)


class ResnetBlock2D(_NoForward):
    def __init__(self, cin, cout, temb, groups, eps):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = nn.Linear(temb, cout)
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)


class _Sampler(_NoForward):
    def __init__(self, c, stride):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=stride, padding=1)


class _Block(_NoForward):
    pass


class TimestepEmbedding(_NoForward):
    def __init__(self, cin, dim):
        super().__init__()
        self.linear_1 = nn.Linear(cin, dim)
        self.linear_2 = nn.Linear(dim, dim)


class UNet2DConditionParams(_NoForward):
    """Module tree with diffusers key names for the config in ``cfg``."""

    def __init__(self, cfg: UNetConfig):
        super().__init__()
        self.cfg = cfg
        self.config = SimpleNamespace(
            sample_size=cfg.sample_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
            block_out_channels=tuple(cfg.block_out_channels), layers_per_block=cfg.layers_per_block,
            attention_head_dim=tuple(cfg.num_heads), cross_attention_dim=cfg.cross_attention_dim,
            norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps)
        G, eps, X, T = cfg.norm_num_groups, cfg.norm_eps, cfg.cross_attention_dim, cfg.time_embed_dim
        c0 = cfg.block_out_channels[0]
        self.conv_in = nn.Conv2d(cfg.in_channels, c0, 3, padding=1)
        self.time_embedding = TimestepEmbedding(c0, T)
        res = {k: (ci, co) for k, ci, co in cfg.resnets()}
        tr = {k: (c, h) for k, _f, c, h in cfg.transformers()}
        n = cfg.num_levels
        self.down_blocks = nn.ModuleList()
        for i in range(n):
            b = _Block()
            b.resnets = nn.ModuleList([ResnetBlock2D(*res[f"down_blocks.{i}.resnets.{j}"], T, G, eps)
                                       for j in range(cfg.layers_per_block)])
            if cfg.down_has_attn(i):
                b.attentions = nn.ModuleList([Transformer2DModel(*tr[f"down_blocks.{i}.attentions.{j}"], X, G)
                                              for j in range(cfg.layers_per_block)])
            if i < n - 1:
                b.downsamplers = nn.ModuleList([_Sampler(cfg.block_out_channels[i], 2)])
            self.down_blocks.append(b)
        m = _Block()
        m.resnets = nn.ModuleList([ResnetBlock2D(*res["mid_block.resnets.0"], T, G, eps),
                                   ResnetBlock2D(*res["mid_block.resnets.1"], T, G, eps)])
        m.attentions = nn.ModuleList([Transformer2DModel(*tr["mid_block.attentions.0"], X, G)])
        self.mid_block = m
        self.up_blocks = nn.ModuleList()
        rev = list(reversed(cfg.block_out_channels))
        for i in range(n):
            b = _Block()
            b.resnets = nn.ModuleList([ResnetBlock2D(*res[f"up_blocks.{i}.resnets.{j}"], T, G, eps)
                                       for j in range(cfg.layers_per_block + 1)])
            if cfg.up_has_attn(i):
                b.attentions = nn.ModuleList([Transformer2DModel(*tr[f"up_blocks.{i}.attentions.{j}"], X, G)
                                              for j in range(cfg.layers_per_block + 1)])
            if i < n - 1:
                b.upsamplers = nn.ModuleList([_Sampler(rev[i], 1)])
            self.up_blocks.append(b)
        self.conv_norm_out = nn.GroupNorm(G, c0, eps=eps)
        self.conv_out = nn.Conv2d(c0, cfg.out_channels, 3, padding=1)

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def enable_gradient_checkpointing(self):   # accepted for API compatibility; inference-only engine
        pass

    # diffusers' UNet2DConditionModel.enable_freeu / disable_freeu (same names and argument order).  The mirror only keeps the
    # setting: the MultiViewUNet that owns this module as its ``base_unet`` hands it to the engine before its next forward.
    freeu = None                # (s1, s2, b1, b2) while enabled
    _freeu_main = False         # set by MultiViewUNet on its base_unet: the UNet of the main pass

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        if not self._freeu_main:
            raise ValueError("enable_freeu: FreeU applies to the main pass only -- call it on MultiViewUNet.base_unet (the image "
                             "encoder's UNet runs without it, as in the reference)")
        self.freeu = check_freeu(s1, s2, b1, b2)

    def disable_freeu(self):
        self.freeu = None

    # tomesd's apply_patch(model, ratio=, max_downsample=) / remove_patch as a pair of the same kind
    tome = None                 # (ratio, max_downsample) while enabled

    def enable_tome(self, ratio: float = 0.5, max_downsample: int = 1):
        if not self._freeu_main:
            raise ValueError("enable_tome: token merging applies to the main pass only -- call it on MultiViewUNet.base_unet (the "
                             "image encoder's pass and the cached reference K/V never merge)")
        tome = check_tome(ratio, max_downsample)
        if tome[0] > 0.0 and self.todo is not None and (self.todo[0] > 1 or self.todo[1] > 1):
            raise ValueError("enable_tome: token downsampling is enabled and the two are alternatives -- disable_todo() first")
        self.tome = tome

    def disable_tome(self):
        self.tome = None

    # token downsampling of the self-attention keys (ToDo): the alternative to token merging
    todo = None                 # (factor, factor_level_2, method) while enabled

    def enable_todo(self, factor: int = 2, factor_level_2: int = 1, method: str = "nearest"):
        if not self._freeu_main:
            raise ValueError("enable_todo: token downsampling applies to the main pass only -- call it on MultiViewUNet.base_unet (the "
                             "image encoder's pass and the cached reference K/V are never downsampled)")
        todo = check_todo(factor, factor_level_2, method)
        if (todo[0] > 1 or todo[1] > 1) and self.tome is not None and self.tome[0] > 0.0:
            raise ValueError("enable_todo: token merging is enabled and the two are alternatives -- disable_tome() first")
        self.todo = todo

    def disable_todo(self):
        self.todo = None


def check_tome(ratio, max_downsample=1):
    """(ratio, max_downsample); ValueError unless 0 <= ratio <= 0.75 and max_downsample is one of 1, 2, 4, 8 (tomesd's)."""
    ratio = float(ratio)
    if not 0.0 <= ratio <= 0.75:
        raise ValueError(f"token merging: ratio must lie in [0, 0.75] (a quarter of the tokens are dst and stay), got {ratio}")
    if isinstance(max_downsample, bool) or max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"token merging: max_downsample must be one of 1, 2, 4, 8, got {max_downsample!r}")
    return ratio, int(max_downsample)


def tome_blocks(cfg, height, width, ratio, max_downsample=1):
    """``{feature name: (H, W, r)}`` of the transformer blocks that merge at a latent of ``height`` x ``width``: tomesd's rule
    ``ceil(sqrt(N0 // N)) <= max_downsample`` with ``r = min(#src, int(N * ratio)) > 0``."""
    import math
    out = {}
    for _, name, _, _ in cfg.transformers():
        part = name.split("_")          # down_block_{i}_attn_{j} | mid_block_attn_0 | up_block_{i}_attn_{j}
        level = int(part[2]) if part[0] == "down" else cfg.num_levels - 1 - (int(part[2]) if part[0] == "up" else 0)
        H, W = height >> level, width >> level
        if H < 2 or W < 2:
            continue
        q = (height * width) // (H * W)
        down = math.isqrt(q - 1) + 1 if q > 0 else 0            # ceil(sqrt(q))
        r = min(H * W - (H // 2) * (W // 2), int(H * W * float(ratio)))
        if down <= max_downsample and r > 0:
            out[name] = (H, W, r)
    return out


TODO_METHODS = ("nearest", "area")          # method of mvd_engine_set_todo / mvd_op_todo_downsample, by index


def check_todo(factor=2, factor_level_2=1, method="nearest"):
    """(factor, factor_level_2, method); ValueError unless both factors are integers in [1, 4] and the method is "nearest" or "area"."""
    for name, f in (("factor", factor), ("factor_level_2", factor_level_2)):
        if isinstance(f, bool) or not isinstance(f, int) or not 1 <= f <= 4:
            raise ValueError(f"token downsampling: {name} must be an integer in [1, 4] (1: untouched), got {f!r}")
    if method not in TODO_METHODS:
        raise ValueError(f"token downsampling: method must be one of {TODO_METHODS}, got {method!r}")
    return int(factor), int(factor_level_2), method


def todo_blocks(cfg, height, width, factor=2, factor_level_2=1):
    """``{feature name: (H, W, f, Nk)}`` of the transformer blocks whose self-attention reads downsampled keys at a latent of
    ``height`` x ``width``: ``down = ceil(sqrt(N0 // N))`` (``tome_blocks``' rule) 1 takes ``factor``, 2 ``factor_level_2``, deeper
    blocks none; a block with ``f == 1``, ``H // f < 1`` or ``W // f < 1`` is untouched.  ``Nk = (H // f) * (W // f)``."""
    import math
    out = {}
    for _, name, _, _ in cfg.transformers():
        part = name.split("_")          # down_block_{i}_attn_{j} | mid_block_attn_0 | up_block_{i}_attn_{j}
        level = int(part[2]) if part[0] == "down" else cfg.num_levels - 1 - (int(part[2]) if part[0] == "up" else 0)
        H, W = height >> level, width >> level
        if H < 1 or W < 1:
            continue
        q = (height * width) // (H * W)
        down = math.isqrt(q - 1) + 1 if q > 0 else 0            # ceil(sqrt(q))
        f = factor if down == 1 else factor_level_2 if down == 2 else 1
        if f > 1 and H // f >= 1 and W // f >= 1:
            out[name] = (H, W, f, (H // f) * (W // f))
    return out


def check_freeu(s1, s2, b1, b2):
    """(s1, s2, b1, b2) as floats; ValueError unless all four are positive and finite."""
    import math
    vals = tuple(float(v) for v in (s1, s2, b1, b2))
    if not all(math.isfinite(v) and v > 0.0 for v in vals):
        raise ValueError(f"FreeU: s1, s2, b1, b2 must be positive and finite, got {vals}")
    return vals
