"""Generator of tests/golden/clip_tokenizer_cases.json: a synthetic CLIP vocabulary + merges, a list of strings and the ids
``transformers.CLIPTokenizer`` gives them (padding="max_length", max_length=77, truncation=True), once with the pad token
``"!"`` (SD-2.1's) and once with ``<|endoftext|>`` (SD-1.x's).  Data only; the transformers version is recorded.

    python tests/golden/make_clip_golden.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "clip_tokenizer_cases.json")

MERGES = ["c a", "ca t</w>", "d o", "do g</w>", "t h", "th e</w>", "a n", "an d</w>", "p h", "ph o", "pho t", "phot o</w>",
          "o f</w>", "' s</w>", "! !</w>", "2 0", "Ã ©</w>", "c a</w>", "o n", "d on", "' t</w>", ". .", ".. .</w>",
          "1 2", "ca f", "caf Ã"]

STRINGS = [
    "",                                                     # empty prompt
    "A photo of the  Cat and dog's café, 2024!!",        # mixed case, whitespace run, contraction, accent, digits, '!'
    "  the\tCAT\n and   THE dog  ",                        # whitespace runs / tabs / newlines
    "don't I'll they've x'd we're I'm cat's 'quoted'",      # contractions
    "caf\u00e9 vs cafe\u0301",                           # precomposed vs decomposed e-acute (NFC)
    "日本語の猫 and 한국어",  # CJK / Hangul letters
    "½ ① x² Ⅷ",                           # number characters: one per piece
    "1234567 3.14 20 2020 120",                             # multi-digit numbers
    "!!!??? ... ,,;; -- (the) [cat]",                       # punctuation runs
    "a<|endoftext|>b the<|endoftext|>",                     # a literal special token
    "<|startoftext|>the cat",                               # ... and the other one
    "cat! dog !the cat",                                    # '!' against letters (pad token '!')
    "the cat!",
    "a  !  b !!",
    "photo-of_the.cat/dog",                                 # punctuation between letters
    "über Ñandú Жук",           # non-ASCII letters, upper case beyond ASCII
    "the cat and the dog " * 30,                            # longer than 77 tokens: eos stays last
    "dog" * 60,                                             # one long word
    "cat " * 75,                                            # exactly at the truncation edge
    "\u00a0the cat\u3000dog",                             # non-ASCII spaces
]


def synthetic_vocab():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    chars = [chr(c) for c in cs]
    toks = chars + [c + "</w>" for c in chars]
    for m in MERGES:
        t = "".join(m.split())
        if t not in toks:
            toks.append(t)
    toks += ["<|startoftext|>", "<|endoftext|>"]
    return {t: i for i, t in enumerate(toks)}


def main():
    import transformers
    from transformers import CLIPTokenizer
    vocab = synthetic_vocab()
    out = {"transformers_version": transformers.__version__, "vocab": vocab, "merges": MERGES, "model_max_length": 77, "sets": []}
    for pad in ("!", "<|endoftext|>"):
        tok = CLIPTokenizer(vocab=dict(vocab), merges=[tuple(m.split()) for m in MERGES], pad_token=pad)
        cases = []
        for s in STRINGS:
            ids = tok(s, padding="max_length", max_length=77, truncation=True).input_ids
            assert len(ids) == 77, (s, len(ids))
            cases.append({"text": s, "ids": [int(i) for i in ids]})
        out["sets"].append({"pad_token": pad, "pad_token_id": int(tok.pad_token_id), "bos_token_id": int(tok.bos_token_id),
                            "eos_token_id": int(tok.eos_token_id), "cases": cases})
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=True, indent=0)
    print(OUT, os.path.getsize(OUT), "bytes", len(STRINGS), "strings x", len(out["sets"]), "pad tokens")


if __name__ == "__main__":
    main()
