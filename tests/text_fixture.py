"""The fake snapshot of tests/hub_fixture.py with a text encoder and a tokenizer written WITHOUT transformers: the UNet / VAE /
scheduler come from ``build_fake_hf_cache(..., with_text_encoder=False)``, ``text_encoder/{config.json, model.safetensors}``
from a seeded ``CLIPTextModelHIP`` state dict and ``tokenizer/{vocab.json, merges.txt, tokenizer_config.json}`` from the same
word list, so the GPU tests of ``text_encoder="hip"`` need no second framework."""
import json
import os

from tests.clip_text_ref import seeded_state_dict
from tests.hub_fixture import VOCAB_WORDS, build_fake_hf_cache

TEXT_CFG = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
                hidden_act="quick_gelu", layer_norm_eps=1e-5)


def fixture_vocab():
    """-> (vocab, merges).  ids: bos 0, eos 1, letter c -> 2 + 2 (c - 'a'), c</w> one more; then every merge product in the
    order of VOCAB_WORDS ("ph" 54, "pho" 55, "phot" 56, "photo</w>" 57, "of</w>" 58, "ch" 59 .. "chair</w>" 62, "re" 63,
    "red</w>" 64, "th" 65, "the</w>" 66, "vi" 67 .. "view</w>" 69, "fr" 70 .. "front</w>" 73); then "!" 74, "!</w>" 75."""
    vocab = {"<|startoftext|>": 0, "<|endoftext|>": 1}
    for ch in "abcdefghijklmnopqrstuvwxyz":
        vocab[ch] = len(vocab)
        vocab[ch + "</w>"] = len(vocab)
    merges = []
    for w in VOCAB_WORDS:
        parts = list(w[:-1]) + [w[-1] + "</w>"]
        while len(parts) > 1:
            m = f"{parts[0]} {parts[1]}"
            if m not in merges:
                merges.append(m)
            parts = [parts[0] + parts[1]] + parts[2:]
            if parts[0] not in vocab:
                vocab[parts[0]] = len(vocab)
    vocab["!"] = len(vocab)
    vocab["!</w>"] = len(vocab)
    return vocab, merges


# hand-derived from the table above (bos, tokens, eos; the tail is the pad id)
EXPECTED_HEADS = {
    "a photo of a red chair": [0, 3, 57, 58, 3, 64, 62, 1],
    "": [0, 1],
    "The  front VIEW of the chair": [0, 66, 73, 69, 58, 66, 62, 1],
    "the red chair!": [0, 66, 64, 62, 74, 1],        # pad token "!": the literal id of "!"; otherwise the word-final "!</w>" = 75
}


def expected_ids(prompt, pad_token, length=77):
    vocab, _ = fixture_vocab()
    head = list(EXPECTED_HEADS[prompt])
    if prompt.endswith("!") and pad_token != "!":
        head[-2] = vocab["!</w>"]
    return head + [vocab[pad_token]] * (length - len(head))


def build_text_snapshot(root, pad_token="<|endoftext|>", seed=0):
    """-> (cache_dir, snapshot_dir, state dicts incl. "text_encoder" (bare keys), text config dict)."""
    from safetensors.torch import save_file
    cache, snap, sds = build_fake_hf_cache(root, with_text_encoder=False, seed=seed)
    vocab, merges = fixture_vocab()
    tok = os.path.join(snap, "tokenizer")
    os.makedirs(tok)
    json.dump(vocab, open(os.path.join(tok, "vocab.json"), "w"))
    open(os.path.join(tok, "merges.txt"), "w").write("#version: 0.2\n" + "\n".join(merges) + "\n")
    json.dump({"model_max_length": 77, "tokenizer_class": "CLIPTokenizer", "bos_token": "<|startoftext|>",
               "eos_token": {"__type": "AddedToken", "content": "<|endoftext|>", "lstrip": False, "normalized": True, "rstrip": False, "single_word": False},
               "unk_token": "<|endoftext|>", "pad_token": pad_token}, open(os.path.join(tok, "tokenizer_config.json"), "w"))
    cfg = dict(TEXT_CFG, vocab_size=len(vocab))
    te = os.path.join(snap, "text_encoder")
    os.makedirs(te)
    json.dump({"architectures": ["CLIPTextModel"], "model_type": "clip_text_model", "bos_token_id": 0, "eos_token_id": 1,
               "pad_token_id": vocab[pad_token], "projection_dim": 64, **cfg}, open(os.path.join(te, "config.json"), "w"))
    sd = seeded_state_dict(cfg, seed=seed + 11)
    save_file({"text_model." + k: v.contiguous() for k, v in sd.items()}, os.path.join(te, "model.safetensors"))   # published spelling
    sds["text_encoder"] = sd
    return cache, snap, sds, cfg
