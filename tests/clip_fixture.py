"""A fake local snapshot of a CLIP model written WITHOUT transformers: ``config.json`` (``text_config`` / ``vision_config`` /
``projection_dim``), ``model.safetensors`` (the combined ``CLIPModel`` state dict: ``text_model.*``, ``vision_model.*``,
``text_projection.weight``, ``visual_projection.weight``, ``logit_scale``), ``preprocessor_config.json`` and the tokenizer
files of tests/text_fixture.py -- what ``mvd_amd.clip_score.CLIPScore(path)`` resolves offline."""
import json
import math
import os

import torch

from tests import clip_vision_ref as V
from tests.clip_text_ref import seeded_state_dict
from tests.text_fixture import TEXT_CFG, fixture_vocab

PROCESSOR = {"image_processor_type": "CLIPImageProcessor", "do_resize": True, "size": {"shortest_edge": 32}, "resample": 3,
             "do_center_crop": True, "crop_size": {"height": 32, "width": 32}, "do_rescale": True, "rescale_factor": 1 / 255,
             "do_normalize": True, "image_mean": list(V.CLIP_MEAN), "image_std": list(V.CLIP_STD), "do_convert_rgb": True}


def build_clip_snapshot(root, seed=0, eos_token_id=1, skip=()):
    """-> (snapshot dir, dict(vision=..., text=..., text_projection=..., vision_cfg=..., text_cfg=..., eos=...)).  ``skip``:
    file names left out."""
    from safetensors.torch import save_file
    snap = os.path.join(str(root), "clip-tiny")
    os.makedirs(snap, exist_ok=True)
    vocab, merges = fixture_vocab()
    tcfg = dict(TEXT_CFG, vocab_size=len(vocab))
    vcfg = dict(V.TINY)
    vsd = V.seeded_vision_state_dict(vcfg, seed=seed + 5)
    tsd = seeded_state_dict(tcfg, seed=seed + 11)
    g = torch.Generator().manual_seed(seed + 17)
    tproj = torch.randn(vcfg["projection_dim"], tcfg["hidden_size"], generator=g) / math.sqrt(tcfg["hidden_size"])
    files = {
        "config.json": lambda p: json.dump({"architectures": ["CLIPModel"], "model_type": "clip", "projection_dim": vcfg["projection_dim"],
                                            "text_config": dict(tcfg, bos_token_id=0, eos_token_id=eos_token_id, pad_token_id=1),
                                            "vision_config": {k: v for k, v in vcfg.items() if k != "projection_dim"}}, open(p, "w")),
        "preprocessor_config.json": lambda p: json.dump(PROCESSOR, open(p, "w")),
        "vocab.json": lambda p: json.dump(vocab, open(p, "w")),
        "merges.txt": lambda p: open(p, "w").write("#version: 0.2\n" + "\n".join(merges) + "\n"),
        "tokenizer_config.json": lambda p: json.dump({"model_max_length": 77, "tokenizer_class": "CLIPTokenizer", "bos_token": "<|startoftext|>",
                                                      "eos_token": "<|endoftext|>", "unk_token": "<|endoftext|>", "pad_token": "<|endoftext|>"}, open(p, "w")),
        "model.safetensors": lambda p: save_file({**{k: v.contiguous() for k, v in vsd.items()}, **{"text_model." + k: v.contiguous() for k, v in tsd.items()},
                                                  "text_projection.weight": tproj.contiguous(), "logit_scale": torch.tensor(2.6592),
                                                  "text_model.embeddings.position_ids": torch.arange(77).unsqueeze(0),
                                                  "vision_model.embeddings.position_ids": torch.arange(V.num_tokens(vcfg)).unsqueeze(0)}, p),
    }
    for name, write in files.items():
        if name not in skip:
            write(os.path.join(snap, name))
    return snap, dict(vision=vsd, text=tsd, text_projection=tproj, vision_cfg=vcfg, text_cfg=tcfg, eos=eos_token_id)
