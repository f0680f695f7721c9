"""CPU restatements behind the CLIP image tower / CLIP score tests (row N7):

* ``pil_bicubic_resize`` / ``preprocess``: PIL's 8-bit ``Image.resize(..., BICUBIC)`` (Resample.c: a horizontal then a vertical
  pass in 2^22 fixed point, each rounded to uint8) and transformers' ``CLIPImageProcessor`` around it, in numpy integers;
  ``tests/test_clip_score_cpu.py`` holds them against recorded and live PIL output byte for byte.
* ``vision_forward`` / ``text_embeds`` / ``clip_scores``: fp32 torch restatement of ``CLIPModel.get_image_features`` /
  ``get_text_features`` (pre-LN ViT, bidirectional attention, ``post_layernorm`` of the class token, bias-free projection; the
  text tower of tests/clip_text_ref.py, pooled at transformers' end-token position), optionally with every GEMM operand and
  weight rounded (bf16 emulation, fp32 residual stream).  Held against transformers itself on the CPU; the GPU tests hold
  the HIP kernels against them.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.clip_text_ref import rel_l2, seeded_state_dict, text_forward  # noqa: F401

PRECISION_BITS = 32 - 8 - 2
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ------------------------------------------------------------------------------- PIL's resize in integers
def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pass_coeffs(n_in, n_out):
    """-> (xmin[n_out], count[n_out], kk[n_out][ksize] int) of one pass."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmins, counts, kk = [], [], np.zeros((n_out, ksize), dtype=np.int64)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        tot = sum(w)
        for x, v in enumerate(w):
            v = v / tot if tot != 0.0 else v
            kk[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmins.append(xmin)
        counts.append(xmax - xmin)
    return xmins, counts, kk


def _pass_last_axis(u8, n_out):
    n_in = u8.shape[-1]
    if n_in == n_out:
        return u8
    xmins, counts, kk = pass_coeffs(n_in, n_out)
    src = u8.astype(np.int64)
    out = np.empty(u8.shape[:-1] + (n_out,), dtype=np.uint8)
    for i in range(n_out):
        acc = (src[..., xmins[i]:xmins[i] + counts[i]] * kk[i, :counts[i]]).sum(-1) + (1 << (PRECISION_BITS - 1))
        out[..., i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_bicubic_resize(u8, oh, ow):
    """u8 (..., H, W) uint8 -> (..., oh, ow) uint8: horizontal pass, then vertical."""
    t = _pass_last_axis(np.asarray(u8), ow)
    return np.swapaxes(_pass_last_axis(np.swapaxes(t, -1, -2), oh), -1, -2)


def resized_size(h, w, s):
    return (s, int(s * w / h)) if h <= w else (int(s * h / w), s)


def resize_crop_u8(u8, size, crop):
    """(..., H, W) uint8 -> the (..., crop, crop) uint8 window the processor normalises."""
    h, w = u8.shape[-2:]
    oh, ow = resized_size(h, w, size)
    r = pil_bicubic_resize(u8, oh, ow)
    top, left = (oh - crop) // 2, (ow - crop) // 2
    return r[..., top:top + crop, left:left + crop]


def normalize_u8(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """transformers' rescale (float64 product, rounded to fp32) and normalize (fp32)."""
    x = (u8.astype(np.float64) * (1 / 255)).astype(np.float32)
    m = np.array(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.array(std, dtype=np.float32).reshape(3, 1, 1)
    return (x - m) / s


def preprocess(u8, size, crop, mean=CLIP_MEAN, std=CLIP_STD):
    return normalize_u8(resize_crop_u8(u8, size, crop), mean, std)


def quantize(x):
    """losses.py:11-13."""
    return ((x.float().clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8)


def patch_rows(pv, P):
    """pixel_values (B, 3, S, S) -> (B * (S / P)^2, 3 P^2) rows in (c, py, px) order."""
    B, C, S, _ = pv.shape
    g = S // P
    return pv.reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P)


# ------------------------------------------------------------------------------- the towers
def _act(h, act):
    if act == "gelu":
        return F.gelu(h)
    if act == "quick_gelu":
        return h * torch.sigmoid(1.702 * h)
    raise ValueError(act)


def vision_forward(sd, pixel_values, cfg, rnd=None):
    """``sd``: ``vision_model.*`` + ``visual_projection.weight``.  -> (last_hidden_state, image_embeds, normalised embeds)."""
    r = rnd or (lambda t: t)
    sd = {k: v.float() for k, v in sd.items()}
    v = "vision_model."
    H, P, heads, eps = cfg["hidden_size"], cfg["patch_size"], cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-5)
    B = pixel_values.shape[0]
    rows = patch_rows(pixel_values.float(), P)
    pe = F.linear(r(rows), r(sd[v + "embeddings.patch_embedding.weight"].reshape(H, -1))).view(B, -1, H)
    x = torch.cat([sd[v + "embeddings.class_embedding"].expand(B, 1, H), pe], 1) + sd[v + "embeddings.position_embedding.weight"]
    x = F.layer_norm(x, (H,), sd[v + "pre_layrnorm.weight"], sd[v + "pre_layrnorm.bias"], eps)
    T, D = x.shape[1], H // heads
    for i in range(cfg["num_hidden_layers"]):
        q = f"{v}encoder.layers.{i}."
        h = r(F.layer_norm(x, (H,), sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"], eps))
        qq = F.linear(h, r(sd[q + "self_attn.q_proj.weight"]), sd[q + "self_attn.q_proj.bias"])
        kk = F.linear(h, r(sd[q + "self_attn.k_proj.weight"]), sd[q + "self_attn.k_proj.bias"])
        vv = F.linear(h, r(sd[q + "self_attn.v_proj.weight"]), sd[q + "self_attn.v_proj.bias"])
        sp = lambda t: r(t).view(B, T, heads, D).transpose(1, 2)   # noqa: E731
        s = sp(qq) @ sp(kk).transpose(-1, -2) / math.sqrt(D)
        o = (r(s.softmax(-1)) @ sp(vv)).transpose(1, 2).reshape(B, T, H)
        x = x + F.linear(r(o), r(sd[q + "self_attn.out_proj.weight"]), sd[q + "self_attn.out_proj.bias"])
        h = r(F.layer_norm(x, (H,), sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"], eps))
        h = _act(F.linear(h, r(sd[q + "mlp.fc1.weight"]), sd[q + "mlp.fc1.bias"]), cfg["hidden_act"])
        x = x + F.linear(r(h), r(sd[q + "mlp.fc2.weight"]), sd[q + "mlp.fc2.bias"])
    pooled = F.layer_norm(x[:, 0], (H,), sd[v + "post_layernorm.weight"], sd[v + "post_layernorm.bias"], eps)
    emb = F.linear(pooled, sd["visual_projection.weight"])
    return x, emb, emb / emb.norm(dim=-1, keepdim=True)


def pooled_position(ids, eos_token_id):
    """transformers' CLIPTextTransformer: argmax of the ids when eos_token_id == 2 (legacy), else the first eos position."""
    if eos_token_id == 2:
        return ids.argmax(-1)
    return (ids == eos_token_id).int().argmax(-1)


def text_embeds(sd, ids, cfg, text_projection, eos_token_id, rnd=None):
    """-> (text_embeds, normalised): the pooled row of ``text_forward`` through the bias-free projection."""
    hid = text_forward(sd, ids, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["hidden_act"], cfg.get("layer_norm_eps", 1e-5), rnd)
    pooled = hid[torch.arange(ids.shape[0]), pooled_position(ids, eos_token_id)]
    emb = F.linear(pooled, text_projection.float())
    return emb, emb / emb.norm(dim=-1, keepdim=True)


def clip_scores(img_norm, txt_norm):
    """torchmetrics 1.6: per-sample 100 cos; the batch value is max(mean, 0)."""
    s = 100.0 * (img_norm.double() * txt_norm.double()).sum(-1)
    return s.float(), torch.clamp(s.mean(), min=0).float()


def bf16_round(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------- configs and seeded weights
TINY = dict(hidden_size=128, intermediate_size=256, projection_dim=64, num_hidden_layers=2, num_attention_heads=2, image_size=32,
            patch_size=8, hidden_act="quick_gelu", layer_norm_eps=1e-5)                      # 17 tokens
P14 = dict(TINY, image_size=28, patch_size=14)                                              # 5 tokens, K 588 -> 640
B32 = dict(hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=2, num_attention_heads=12, image_size=224,
           patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5)                      # ViT-B/32 geometry, 50 tokens
L14 = dict(hidden_size=1024, intermediate_size=4096, projection_dim=768, num_hidden_layers=4, num_attention_heads=16, image_size=224,
           patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)                      # ViT-L/14 geometry, 257 tokens
L14_FULL = dict(L14, num_hidden_layers=24)


def num_tokens(cfg):
    return 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2


def seeded_vision_state_dict(cfg, seed=0):
    """The layers as tests/clip_text_ref.py seeds them (nothing trivially zero); class / position embeddings N(0, 1) * 0.3 so
    the pre-LayerNorm sees the patch term and the tables at comparable size; patch and projection matrices N(0, 1 / fan_in).
    Keys: ``vision_model.*`` + ``visual_projection.weight``."""
    H, P = cfg["hidden_size"], cfg["patch_size"]
    layers = seeded_state_dict(dict(cfg, vocab_size=1, max_position_embeddings=1), seed=seed)
    g = torch.Generator().manual_seed(seed + 7919)
    n = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    sd = {"vision_model." + k: v for k, v in layers.items() if k.startswith("encoder.")}
    sd["vision_model.embeddings.class_embedding"] = 0.3 * n(H)
    sd["vision_model.embeddings.patch_embedding.weight"] = n(H, 3, P, P) / math.sqrt(3 * P * P)
    sd["vision_model.embeddings.position_embedding.weight"] = 0.3 * n(num_tokens(cfg), H)
    for name in ("pre_layrnorm", "post_layernorm"):
        sd[f"vision_model.{name}.weight"] = 1 + 0.2 * n(H)
        sd[f"vision_model.{name}.bias"] = 0.1 * n(H)
    sd["visual_projection.weight"] = n(cfg["projection_dim"], H) / math.sqrt(H)
    return sd


def seeded_pixel_values(cfg, batch, seed=0):
    """Shaped like normalised images: N(0, 1) with smooth structure per channel plus noise."""
    g = torch.Generator().manual_seed(100 + seed)
    S = cfg["image_size"]
    low = F.interpolate(torch.randn(batch, 3, max(S // 8, 1), max(S // 8, 1), generator=g), size=(S, S), mode="bilinear", align_corners=False)
    return (low + 0.5 * torch.randn(batch, 3, S, S, generator=g)).contiguous()
