"""CLIP's byte-level BPE tokenizer in plain Python: what ``transformers.CLIPTokenizer`` gives
/root/reference/src/models/pipeline.py:52-75 (``tokenizer(prompt, padding="max_length", max_length=..., truncation=True,
return_tensors="pt").input_ids``), read from the ``tokenizer/`` directory of a local snapshot.  Standard library + torch
only: no ``transformers``, no ``tokenizers``, no ``regex``.

Algorithm (checked against transformers' tokenizer on the golden cases of tests/golden/clip_tokenizer_cases.json):

1. the raw text is split on the literal special-token strings (bos, eos and the pad token -- SD-2.1 pads with ``"!"``, and
   the reference tokenizer emits the pad id for every ``!`` of a prompt instead of merging it); each match is its id;
2. every other segment: NFC, whitespace runs collapsed to one space, stripped, lower-cased;
3. pre-tokenised, leftmost match with the first alternative winning, by
   ``'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+`` (one number character per piece; categories from
   ``unicodedata``);
4. UTF-8 bytes -> CLIP's byte-to-unicode table, the last symbol gets ``</w>``, merges applied by rank;
5. ``[bos] + ids[:max_length - 2] + [eos]``, padded with the pad id to ``max_length``.

``ftfy`` text fixing, attention masks and case variants of the special strings are out of scope.
"""
from __future__ import annotations

import json
import os
import re
import unicodedata
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple, Union

_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def bytes_to_unicode() -> Dict[int, str]:
    """CLIP / GPT-2's reversible byte -> printable character table."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def _kind(ch: str) -> str:
    """'L' letter, 'N' number, 'S' whitespace, 'O' anything else -- the classes of the pre-tokeniser pattern."""
    if ch.isspace():
        return "S"
    cat = unicodedata.category(ch)
    return cat[0] if cat[0] in "LN" else "O"


def pretokenize(text: str) -> List[str]:
    """Leftmost / first-alternative-wins scan of ``'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+``."""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch == "'":
            c = next((c for c in _CONTRACTIONS if text.startswith(c, i)), None)
            if c is not None:
                out.append(c)
                i += len(c)
                continue
        k = _kind(ch)
        if k == "S":
            i += 1
        elif k == "N":
            out.append(ch)
            i += 1
        else:
            j = i + 1
            while j < n and _kind(text[j]) == k:
                j += 1
            out.append(text[i:j])
            i = j
    return out


def _token_str(v) -> str:
    return v["content"] if isinstance(v, dict) else v


class CLIPTokenizerLite:
    """``vocab``: token -> id; ``merges``: ranked ``(a, b)`` pairs.  Called like the transformers tokenizer."""

    def __init__(self, vocab: Dict[str, int], merges: Sequence[Tuple[str, str]], bos_token: str = "<|startoftext|>",
                 eos_token: str = "<|endoftext|>", unk_token: str = "<|endoftext|>", pad_token: str = "<|endoftext|>",
                 model_max_length: int = 77):
        self.encoder = dict(vocab)
        self.bpe_ranks = {tuple(m): i for i, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        self.bos_token, self.eos_token, self.unk_token, self.pad_token = bos_token, eos_token, unk_token, pad_token
        for name in ("bos", "eos", "unk", "pad"):
            tok = getattr(self, f"{name}_token")
            if tok not in self.encoder:
                raise ValueError(f"CLIPTokenizerLite: {name} token {tok!r} is not in the vocabulary")
            setattr(self, f"{name}_token_id", self.encoder[tok])
        self.model_max_length = int(model_max_length)
        specials = sorted({bos_token, eos_token, pad_token}, key=len, reverse=True)
        self._special_re = re.compile("(" + "|".join(re.escape(t) for t in specials) + ")")
        self._specials = set(specials)
        self._cache: Dict[str, List[str]] = {}

    @classmethod
    def from_pretrained(cls, path: str, **_ignored) -> "CLIPTokenizerLite":
        """``vocab.json`` + ``merges.txt`` (+ ``tokenizer_config.json`` / ``special_tokens_map.json``) of a local directory."""
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        merges = []
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            for i, line in enumerate(f.read().split("\n")):
                if (i == 0 and line.startswith("#version")) or not line.strip():
                    continue
                a, b = line.split()
                merges.append((a, b))
        cfg = {}
        for name in ("special_tokens_map.json", "tokenizer_config.json"):      # the config wins
            fn = os.path.join(path, name)
            if os.path.exists(fn):
                with open(fn, encoding="utf-8") as f:
                    cfg.update(json.load(f))
        kw = {k: _token_str(cfg[k]) for k in ("bos_token", "eos_token", "unk_token", "pad_token") if cfg.get(k) is not None}
        mml = cfg.get("model_max_length", 77)
        if not isinstance(mml, int) or mml <= 0 or mml > 1 << 20:
            mml = 77
        return cls(vocab, merges, model_max_length=mml, **kw)

    # ------------------------------------------------------------------ BPE
    def _bpe(self, word: str) -> List[str]:
        hit = self._cache.get(word)
        if hit is not None:
            return hit
        sym = list(word[:-1]) + [word[-1] + "</w>"]
        big = 1 << 60
        while len(sym) > 1:
            rank, pair = min(((self.bpe_ranks.get(p, big), p) for p in zip(sym, sym[1:])), key=lambda t: t[0])
            if rank == big:
                break
            a, b = pair
            out, i = [], 0
            while i < len(sym):
                if i + 1 < len(sym) and sym[i] == a and sym[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(sym[i])
                    i += 1
            sym = out
        self._cache[word] = sym
        return sym

    def tokenize_ids(self, text: str) -> List[int]:
        """ids of ``text`` without bos / eos / padding."""
        ids: List[int] = []
        for seg in self._special_re.split(text):
            if seg in self._specials:
                ids.append(self.encoder[seg])
                continue
            seg = " ".join(unicodedata.normalize("NFC", seg).split()).lower()
            for piece in pretokenize(seg):
                word = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
                ids.extend(self.encoder.get(s, self.unk_token_id) for s in self._bpe(word))
        return ids

    def encode(self, text: str, max_length: int = None, padding=False, truncation: bool = False) -> List[int]:
        L = self.model_max_length if max_length is None else int(max_length)
        ids = self.tokenize_ids(text)
        if truncation:
            ids = ids[:max(L - 2, 0)]
        ids = [self.bos_token_id] + ids + [self.eos_token_id]
        if padding == "max_length":
            ids = ids + [self.pad_token_id] * (L - len(ids))
        return ids

    def __call__(self, text: Union[str, List[str]], padding=False, max_length: int = None, truncation: bool = False,
                 return_tensors: str = None, **_ignored):
        single = isinstance(text, str)
        rows = [self.encode(t, max_length, padding, truncation) for t in ([text] if single else list(text))]
        if padding is True or padding == "longest":
            m = max(len(r) for r in rows)
            rows = [r + [self.pad_token_id] * (m - len(r)) for r in rows]
        if return_tensors == "pt":
            import torch
            if len({len(r) for r in rows}) != 1:
                raise ValueError("CLIPTokenizerLite: rows of different length cannot form a tensor: use padding='max_length'")
            return SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.long))
        if return_tensors is not None:
            raise ValueError(f"CLIPTokenizerLite: return_tensors={return_tensors!r} (only 'pt')")
        return SimpleNamespace(input_ids=rows[0] if single else rows)
