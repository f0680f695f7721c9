"""Row N5 without a GPU: the CPU restatement of the CLIP text transformer against transformers' own ``CLIPTextModel``, the
native tokenizer against ids recorded from ``transformers.CLIPTokenizer`` (tests/golden/clip_tokenizer_cases.json) and,
when the package imports, against the live tokenizer; state-dict key spellings and config validation of
``CLIPTextModelHIP``; and that none of it needs transformers to import."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import clip_text_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_tokenizer_cases.json")


# ------------------------------------------------------------------------------- restatement vs transformers
@pytest.mark.parametrize("kind", ["tiny", "sd21"])
def test_restatement_matches_transformers(kind):
    """rel-L2 <= 1e-5: ~17x the fp32 reordering noise measured between the two (4.3e-7 tiny / 5.9e-7 SD-2.1 size), three
    orders of magnitude below what a wrong mask, activation form or eps produces."""
    tr = pytest.importorskip("transformers")
    cfg = R.TINY if kind == "tiny" else R.SD21
    tc = tr.CLIPTextConfig(projection_dim=64, pad_token_id=1, bos_token_id=0, eos_token_id=2, **cfg)
    m = tr.CLIPTextModel(tc).eval().float()
    sd = R.seeded_state_dict(cfg, seed=3)
    own = m.state_dict()
    prefix = "text_model." if any(k.startswith("text_model.") for k in own) else ""
    res = m.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith("position_ids") for k in res.missing_keys), res
    ids = R.prompt_like_ids(cfg, 2, seed=1)
    assert (ids[:, -1] == 0).all(), "the ids carry a pad tail of id 0"
    with torch.no_grad():
        want = m(input_ids=ids)[0]
        got = R.text_forward(sd, ids, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["hidden_act"], cfg["layer_norm_eps"])
    rel = R.rel_l2(got, want)
    print(f"{kind}: restatement vs transformers rel-L2 {rel:.3e}, max-abs {float((got - want).abs().max()):.3e}, rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert torch.isfinite(got).all() and rel <= 1e-5, rel


# ------------------------------------------------------------------------------- tokenizer
def _golden():
    return json.load(open(GOLDEN, encoding="utf-8"))


def _lite(d, pad):
    from mvd_amd.clip_tokenizer import CLIPTokenizerLite
    return CLIPTokenizerLite(d["vocab"], [tuple(m.split()) for m in d["merges"]], pad_token=pad, model_max_length=d["model_max_length"])


def test_tokenizer_matches_golden():
    d = _golden()
    assert len(d["sets"]) == 2 and all(len(s["cases"]) >= 20 for s in d["sets"])
    for st in d["sets"]:
        tok = _lite(d, st["pad_token"])
        assert (tok.pad_token_id, tok.bos_token_id, tok.eos_token_id) == (st["pad_token_id"], st["bos_token_id"], st["eos_token_id"])
        assert tok.model_max_length == 77
        for c in st["cases"]:
            out = tok(c["text"], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
            assert out.dtype == torch.long and out.shape == (1, 77)
            assert out[0].tolist() == c["ids"], (st["pad_token"], c["text"][:50])
        texts = [c["text"] for c in st["cases"]]
        batch = tok(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        assert batch.tolist() == [c["ids"] for c in st["cases"]]


def test_golden_covers_the_required_strings():
    d = _golden()
    texts = [c["text"] for c in d["sets"][0]["cases"]]
    eos = d["sets"][0]["eos_token_id"]
    assert "" in texts and any("<|endoftext|>" in t for t in texts) and any("!" in t for t in texts)
    assert any("é" in t and "é" in t for t in texts) and any("日" in t for t in texts)
    assert any("½" in t and "①" in t and "²" in t for t in texts) and any("1234567" in t for t in texts)
    assert any("don't" in t for t in texts) and any("..." in t for t in texts)
    long_cases = [c for c in d["sets"][0]["cases"] if len(c["text"]) > 400]
    assert long_cases and all(c["ids"][-1] == eos and len(c["ids"]) == 77 for c in long_cases)


def test_tokenizer_matches_transformers_live():
    tr = pytest.importorskip("transformers")
    d = _golden()
    for pad in ("!", "<|endoftext|>"):
        ref = tr.CLIPTokenizer(vocab=dict(d["vocab"]), merges=[tuple(m.split()) for m in d["merges"]], pad_token=pad)
        tok = _lite(d, pad)
        for c in d["sets"][0]["cases"]:
            want = ref(c["text"], padding="max_length", max_length=77, truncation=True).input_ids
            got = tok(c["text"], padding="max_length", max_length=77, truncation=True).input_ids
            assert got == list(want), (pad, c["text"][:50])


def test_tokenizer_from_files_and_unknown_symbols(tmp_path):
    from mvd_amd.clip_tokenizer import CLIPTokenizerLite
    d = _golden()
    json.dump(d["vocab"], open(tmp_path / "vocab.json", "w"))
    open(tmp_path / "merges.txt", "w", encoding="utf-8").write("#version: 0.2\n" + "\n".join(d["merges"]) + "\n")
    json.dump({"pad_token": {"content": "!"}, "bos_token": "<|startoftext|>"}, open(tmp_path / "special_tokens_map.json", "w"))
    tok = CLIPTokenizerLite.from_pretrained(str(tmp_path))
    assert tok.pad_token == "!" and tok.model_max_length == 77          # the default
    st = next(s for s in d["sets"] if s["pad_token"] == "!")
    for c in st["cases"][:6]:
        assert tok(c["text"], padding="max_length", max_length=77, truncation=True).input_ids == c["ids"]
    small = {k: v for k, v in d["vocab"].items() if k not in ("z", "z</w>")}
    t2 = CLIPTokenizerLite(small, [], pad_token="<|endoftext|>")
    ids = t2("zz", padding="max_length", max_length=8, truncation=True).input_ids
    assert ids == [t2.bos_token_id, t2.unk_token_id, t2.unk_token_id, t2.eos_token_id] + [t2.pad_token_id] * 4


# ------------------------------------------------------------------------------- CLIPTextModelHIP as a container
def test_both_key_spellings_load_and_bad_configs_raise():
    from mvd_amd._lib import MvdError
    from mvd_amd.text_encoder import CLIPTextConfigLite, CLIPTextModelHIP, pack_text
    cfg = dict(R.TINY, vocab_size=64)
    sd = R.seeded_state_dict(cfg, seed=5)
    a, b = CLIPTextModelHIP(CLIPTextConfigLite(**cfg)), CLIPTextModelHIP(CLIPTextConfigLite(**cfg))
    r1 = a.load_state_dict(sd)
    pref = {"text_model." + k: v for k, v in sd.items()}
    pref["text_model.embeddings.position_ids"] = torch.arange(77)[None]
    r2 = b.load_state_dict(pref)
    assert not r1.missing_keys and not r1.unexpected_keys and not r2.missing_keys and not r2.unexpected_keys
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb) and torch.equal(va, sd[ka])
    assert set(a.state_dict()) == set(sd)
    packed = pack_text(a.state_dict(), a.config, "cpu")
    H = cfg["hidden_size"]
    assert packed["layers.0.qkv.w"].shape == (3 * H, H) and packed["layers.0.qkv.w"].dtype == torch.bfloat16
    assert packed["tok"].dtype == torch.float32 and packed["layers.1.fc1.b"].dtype == torch.float32
    with pytest.raises(MvdError, match="hidden_act"):
        CLIPTextModelHIP(CLIPTextConfigLite(**dict(cfg, hidden_act="relu")))
    with pytest.raises(MvdError, match="head dimension"):
        CLIPTextModelHIP(CLIPTextConfigLite(**dict(cfg, num_attention_heads=4)))
    with pytest.raises(MvdError):
        a(torch.full((1, 5), 64))                    # an id == vocab_size: refused on the host, before any device work
    with pytest.raises(MvdError):
        a(torch.zeros(1, 78, dtype=torch.long))      # beyond max_position_embeddings


def test_c_abi_validates_on_the_host():
    import ctypes as C
    from mvd_amd import _lib as L
    lib = L.lib()

    def mk(**kw):
        c = L.mvd_text_config_t()
        base = dict(vocab_size=100, hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, max_positions=77,
                    layer_norm_eps=1e-5, act=1)
        base.update(kw)
        for k, v in base.items():
            setattr(c, k, v)
        h = C.c_void_p()
        return lib.mvd_text_create(C.byref(c), C.byref(h)), h

    for bad in (dict(num_heads=4), dict(hidden_size=96, num_heads=1), dict(max_positions=97), dict(act=2), dict(intermediate_size=500)):
        rc, _ = mk(**bad)
        assert rc < 0 and L.last_error(), bad
    rc, h = mk()
    assert rc == 0
    w1, w3 = lib.mvd_text_workspace_bytes(h, 1, 77), lib.mvd_text_workspace_bytes(h, 3, 77)
    assert 0 < w1 < w3
    assert lib.mvd_text_workspace_bytes(h, 1, 78) < 0 and "max_positions" in L.last_error()
    ids = (C.c_int32 * 77)()
    out = (C.c_float * 8)()
    assert lib.mvd_text_encode(h, ids, 1, 78, out, None) < 0 and "max_positions" in L.last_error()
    assert lib.mvd_text_encode(h, ids, 1, 77, out, None) < 0 and "missing weight slot" in L.last_error()   # before any launch
    lib.mvd_text_destroy(h)


def test_pipeline_keyword_is_validated(tmp_path):
    from mvd_amd._lib import MvdError
    from mvd_amd.pipeline import _native_text_components, _optional_components
    with pytest.raises(MvdError, match="lacks"):
        os.makedirs(tmp_path / "snap" / "text_encoder")
        _native_text_components(str(tmp_path / "snap"))
    with pytest.raises(MvdError):
        _optional_components(None, torch.float32, "hip")
    assert _optional_components(None, torch.float32) == (None, None, None)


# ------------------------------------------------------------------------------- no transformers needed
def test_native_modules_import_without_transformers():
    code = (
        "import sys, json\n"
        "sys.modules['transformers'] = None\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import mvd_amd.text_encoder, mvd_amd.clip_tokenizer\n"
        "from mvd_amd.clip_tokenizer import CLIPTokenizerLite\n"
        f"d = json.load(open({GOLDEN!r}, encoding='utf-8'))\n"
        "n = 0\n"
        "for st in d['sets']:\n"
        "    tok = CLIPTokenizerLite(d['vocab'], [tuple(m.split()) for m in d['merges']], pad_token=st['pad_token'])\n"
        "    for c in st['cases']:\n"
        "        assert tok(c['text'], padding='max_length', max_length=77, truncation=True).input_ids == c['ids'], c['text'][:40]\n"
        "        n += 1\n"
        "assert sys.modules['transformers'] is None and 'tokenizers' not in sys.modules and 'regex' not in sys.modules\n"
        "print('ok', n)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok 40"), r.stdout + r.stderr
