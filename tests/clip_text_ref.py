"""fp32 torch restatement of the CLIP text transformer (``last_hidden_state`` of transformers' ``CLIPTextModel``), the CPU
reference of the text-encoder tests (row N5):

    x   = token_embedding[ids] + position_embedding[0:T]
    per layer:  h = LN1(x); q,k,v = h.Wq^T+bq, h.Wk^T+bk, h.Wv^T+bv
                a = softmax(q.k^T / sqrt(64) + causal) . v      per head        (key j visible to query i iff j <= i)
                x = x + a.Wo^T + bo;  h = LN2(x); h = act(h.W1^T + b1); x = x + h.W2^T + b2
    out = final_layer_norm(x)

No padding mask (the reference pipeline passes ``input_ids`` only).  ``tests/test_text_encoder_cpu.py`` holds it against
transformers itself; the GPU tests hold the HIP encoder against it.
"""
import math

import torch
import torch.nn.functional as F


def text_forward(sd, ids, num_layers, num_heads, act, eps=1e-5, rnd=None):
    """``sd``: state dict with transformers' key names (with or without ``text_model.``); ``ids`` (B, T) long.
    ``rnd``: optional rounding applied to every GEMM operand and weight (bf16 emulation; the residual stream stays fp32)."""
    r = rnd or (lambda t: t)
    p = "text_model." if any(k.startswith("text_model.") for k in sd) else ""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    B, T = ids.shape
    x = sd[p + "embeddings.token_embedding.weight"][ids] + sd[p + "embeddings.position_embedding.weight"][:T]
    mask = torch.full((T, T), float("-inf")).triu(1)
    for i in range(num_layers):
        q = f"{p}encoder.layers.{i}."
        h = r(F.layer_norm(x, x.shape[-1:], sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"], eps))
        qq = F.linear(h, r(sd[q + "self_attn.q_proj.weight"]), sd[q + "self_attn.q_proj.bias"])
        kk = F.linear(h, r(sd[q + "self_attn.k_proj.weight"]), sd[q + "self_attn.k_proj.bias"])
        vv = F.linear(h, r(sd[q + "self_attn.v_proj.weight"]), sd[q + "self_attn.v_proj.bias"])
        D = x.shape[-1] // num_heads
        sp = lambda t: r(t).view(B, T, num_heads, D).transpose(1, 2)   # noqa: E731
        s = sp(qq) @ sp(kk).transpose(-1, -2) / math.sqrt(D) + mask
        o = (r(s.softmax(-1)) @ sp(vv)).transpose(1, 2).reshape(B, T, -1)
        x = x + F.linear(r(o), r(sd[q + "self_attn.out_proj.weight"]), sd[q + "self_attn.out_proj.bias"])
        h = r(F.layer_norm(x, x.shape[-1:], sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"], eps))
        h = F.linear(h, r(sd[q + "mlp.fc1.weight"]), sd[q + "mlp.fc1.bias"])
        if act == "gelu":
            h = F.gelu(h)
        elif act == "quick_gelu":
            h = h * torch.sigmoid(1.702 * h)
        else:
            raise ValueError(act)
        x = x + F.linear(r(h), r(sd[q + "mlp.fc2.weight"]), sd[q + "mlp.fc2.bias"])
    return F.layer_norm(x, x.shape[-1:], sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)


TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
SD21 = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
            max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5)


def seeded_state_dict(cfg, seed=0):
    """Nothing trivially zero: LayerNorm gains 1 + 0.2 N(0,1), every bias 0.1 N(0,1), matrices N(0, 1/fan_in); embedding
    tables N(0, 0.02^2) / N(0, 0.01^2) (transformers' own initialisation).  Bare key names."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    sd = {"embeddings.token_embedding.weight": 0.02 * n(cfg["vocab_size"], H),
          "embeddings.position_embedding.weight": 0.01 * n(cfg["max_position_embeddings"], H)}

    def ln(key):
        sd[key + ".weight"] = 1 + 0.2 * n(H)
        sd[key + ".bias"] = 0.1 * n(H)

    def lin(key, o, i):
        sd[key + ".weight"] = n(o, i) / math.sqrt(i)
        sd[key + ".bias"] = 0.1 * n(o)

    for l in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{l}"
        ln(p + ".layer_norm1")
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(f"{p}.self_attn.{nm}", H, H)
        ln(p + ".layer_norm2")
        lin(p + ".mlp.fc1", I, H)
        lin(p + ".mlp.fc2", H, I)
    ln("final_layer_norm")
    return sd


def prompt_like_ids(cfg, batch, seed=0, seq_len=None):
    """bos, a random body, eos, then a pad tail of id 0 (SD-2.1 pads with id 0), lengths varying per row."""
    T = seq_len or cfg["max_position_embeddings"]
    V = cfg["vocab_size"]
    g = torch.Generator().manual_seed(1000 + seed)
    ids = torch.randint(1, V - 2, (batch, T), generator=g)
    ids[:, 0] = V - 2
    for b in range(batch):
        end = min(T - 1, 5 + (7 * b + 3 * seed) % max(T - 6, 1))
        ids[b, end] = V - 1
        ids[b, end + 1:] = 0
    return ids


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())
