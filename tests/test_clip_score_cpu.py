"""Row N7 without a GPU: the CPU restatements of tests/clip_vision_ref.py against transformers (fp32 rounding) and against
PIL (byte for byte, recorded and live), state-dict loading of ``CLIPVisionModelHIP``, host-side validation of the C ABI,
``CLIPScore`` on fake snapshots, and ``import mvd_amd.clip_score`` with transformers blocked.

Measured here (seeded weights, fp32): image_embeds / text_embeds of the restatement against transformers 5.15 differ by
at most 6.3e-7 relative to max|ref| (tiny and ViT-B/32 geometry); the bound below is 1e-5."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import clip_vision_ref as V
from tests.clip_fixture import build_clip_snapshot
from tests.clip_text_ref import seeded_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_preprocess_cases.npz")
SMALL = ("r40x56", "r56x40", "r17x23", "r32x32", "r64x64", "r5x7")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------- the resize restatement
def test_resize_restatement_matches_the_recorded_pil_output_exactly(golden):
    for name in SMALL:
        got = V.preprocess(golden[name + "_in"], 32, 32)
        assert got.dtype == np.float32 and np.array_equal(got, golden[name + "_pv"]), name
    assert np.array_equal(V.resize_crop_u8(golden["big_in"], 224, 224), golden["big_u8"])
    assert np.array_equal(V.quantize(torch.from_numpy(golden["quant_in"])).numpy(), golden["quant_u8"])


@pytest.mark.parametrize("h,w,oh,ow", [(40, 56, 32, 44), (100, 64, 350, 224), (17, 23, 32, 43), (224, 224, 224, 224), (300, 224, 43, 32),
                                       (5, 7, 32, 44), (512, 512, 224, 224)])
def test_resize_restatement_matches_live_pil(h, w, oh, ow):
    Image = pytest.importorskip("PIL.Image")
    a = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC))
    got = V.pil_bicubic_resize(a.transpose(2, 0, 1), oh, ow).transpose(1, 2, 0)
    assert np.array_equal(got, want)


def test_resize_accumulator_stays_in_32_bits():
    """255 * sum |kk| + 2^21 < 2^31 for the scales in use (the kernel accumulates in int32; the host asserts the same)."""
    for n_in, n_out in [(768, 224), (512, 224), (4096, 224), (17, 32), (5, 32)]:
        _, _, kk = V.pass_coeffs(n_in, n_out)
        assert 255 * int(np.abs(kk).sum(1).max()) + (1 << 21) < 1 << 31


# ------------------------------------------------------------------------------- the towers against transformers
def _hf_clip(vcfg, tcfg, eos):
    tr = pytest.importorskip("transformers")
    cfg = tr.CLIPConfig(text_config=dict(tcfg, eos_token_id=eos, bos_token_id=1, pad_token_id=0),
                        vision_config={k: v for k, v in vcfg.items() if k != "projection_dim"}, projection_dim=vcfg["projection_dim"])
    return tr.CLIPModel(cfg).eval()


def _features(out):
    return getattr(out, "pooler_output", out)       # (recent transformers return an output object, older ones the tensor)


@pytest.mark.parametrize("kind", ["tiny", "b32"])
def test_restatement_matches_transformers(kind):
    vcfg = V.TINY if kind == "tiny" else V.B32
    tcfg = dict(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    vsd, tsd = V.seeded_vision_state_dict(vcfg, seed=1), seeded_state_dict(tcfg, seed=2)
    tproj = torch.randn(vcfg["projection_dim"], tcfg["hidden_size"], generator=torch.Generator().manual_seed(3)) / 11.3
    pv = V.seeded_pixel_values(vcfg, 2, seed=4)
    # ids where the two pooling rules pick different rows: the largest id (998) sits in front of the end token
    for eos in (2, 500):
        ids = torch.randint(3, 400, (2, 12), generator=torch.Generator().manual_seed(5))
        ids[:, 0] = 1
        ids[0, 3], ids[1, 5] = 998, 998
        ids[0, 7], ids[1, 9] = eos, eos
        ids[0, 8:], ids[1, 10:] = 0, 0
        want_pos = [3, 5] if eos == 2 else [7, 9]
        assert V.pooled_position(ids, eos).tolist() == want_pos and V.pooled_position(ids, 502 - eos).tolist() != want_pos
        model = _hf_clip(vcfg, tcfg, eos)
        res = model.load_state_dict({**vsd, **{"text_model." + k: v for k, v in tsd.items()}, "text_projection.weight": tproj}, strict=False)
        assert not res.unexpected_keys and all(k.endswith("position_ids") or k == "logit_scale" for k in res.missing_keys), res
        with torch.no_grad():
            hf_img = _features(model.get_image_features(pixel_values=pv))
            hf_txt = _features(model.get_text_features(input_ids=ids))
            _, img, _ = V.vision_forward(vsd, pv, vcfg)
            txt, _ = V.text_embeds(tsd, ids, tcfg, tproj, eos)
        ei = ((img - hf_img).abs().max() / hf_img.abs().max()).item()
        et = ((txt - hf_txt).abs().max() / hf_txt.abs().max()).item()
        print(f"{kind} eos {eos}: image_embeds max-abs / max|ref| {ei:.3e}, text_embeds {et:.3e}")
        assert ei <= 1e-5 and et <= 1e-5, (kind, eos, ei, et)


def test_preprocess_restatement_matches_the_live_processor():
    tr = pytest.importorskip("transformers")
    pytest.importorskip("PIL.Image")
    proc = tr.CLIPImageProcessorPil(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    u8 = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 3, 45, 37), dtype=np.uint8))
    want = proc(images=u8, return_tensors="pt")["pixel_values"].numpy()
    assert np.array_equal(V.preprocess(u8.numpy(), 32, 32), want)


def test_bf16_emulation_stays_under_a_third_of_the_gpu_bound():
    """The GPU encoder tests bound rel-L2 at the text tower's 2e-2 because the bf16-operand restatement stays under a third
    of it (measured: 3.1e-3 .. 5.0e-3 over the five configs); the small configs are re-measured here."""
    for cfg, B in ((V.TINY, 3), (V.P14, 2), (V.B32, 1)):
        sd, pv = V.seeded_vision_state_dict(cfg, seed=3), V.seeded_pixel_values(cfg, B, seed=B)
        with torch.no_grad():
            ref, emu = V.vision_forward(sd, pv, cfg), V.vision_forward(sd, pv, cfg, rnd=V.bf16_round)
        rels = [V.rel_l2(e, r) for e, r in zip(emu, ref)]
        print(f"bf16 emulation, {V.num_tokens(cfg)} tokens: rel-L2 hidden {rels[0]:.3e}, embeds {rels[1]:.3e}, normalised {rels[2]:.3e}")
        assert max(rels) <= 2e-2 / 3


# ------------------------------------------------------------------------------- the parameter container
def test_state_dict_loading_both_spellings_and_a_combined_file(tmp_path):
    from mvd_amd.text_encoder import CLIPTextConfigLite, CLIPTextModelHIP
    from mvd_amd.vision_encoder import CLIPVisionConfigLite, CLIPVisionModelHIP, pack_vision, split_clip_state_dict
    cfg = CLIPVisionConfigLite(**V.P14)
    sd = V.seeded_vision_state_dict(V.P14, seed=1)
    m = CLIPVisionModelHIP(cfg)
    res = m.load_state_dict(dict(sd, **{"vision_model.embeddings.position_ids": torch.arange(5).unsqueeze(0)}))
    assert not res.missing_keys and not res.unexpected_keys
    assert set(m.state_dict()) == set(sd)
    bare = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}
    m2 = CLIPVisionModelHIP(cfg)
    res = m2.load_state_dict(bare)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]) and torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        CLIPVisionModelHIP(cfg).load_state_dict({k: v for k, v in sd.items() if "post_layernorm" not in k})
    # packing: the patch weight as [H][Kp] rows in (c, py, px) order, zero padded 588 -> 640; q rows carry QSCALE
    from mvd_amd.packing import QSCALE
    packed = pack_vision(m.state_dict(), cfg, "cpu")
    assert cfg.patch_k == 640 and packed["patch.w"].shape == (128, 640) and packed["patch.w"].dtype == torch.bfloat16
    assert torch.equal(packed["patch.w"][:, :588].float(), sd["vision_model.embeddings.patch_embedding.weight"].reshape(128, 588).to(torch.bfloat16).float())
    assert not packed["patch.w"][:, 588:].any()
    q = sd["vision_model.encoder.layers.0.self_attn.q_proj.weight"]
    assert torch.equal(packed["layers.0.qkv.w"][:128].float(), (q * QSCALE).to(torch.bfloat16).float())
    assert packed["proj.w"].dtype == torch.float32 and packed["pos"].shape == (5, 128)
    # a combined CLIPModel file -> the two towers
    snap, parts = build_clip_snapshot(tmp_path)
    from safetensors.torch import load_file
    vsd, tsd, tproj = split_clip_state_dict(load_file(os.path.join(snap, "model.safetensors")))
    mv, mt = CLIPVisionModelHIP(CLIPVisionConfigLite(**parts["vision_cfg"])), CLIPTextModelHIP(CLIPTextConfigLite(**parts["text_cfg"]))
    assert not mv.load_state_dict(vsd).missing_keys and not mt.load_state_dict(tsd).missing_keys
    assert torch.equal(tproj, parts["text_projection"])
    assert torch.equal(mv.state_dict()["visual_projection.weight"], parts["vision"]["visual_projection.weight"])


def test_bad_configs_raise_on_the_host():
    from mvd_amd._lib import MvdError
    from mvd_amd.vision_encoder import CLIPImageProcessorLite, CLIPVisionConfigLite, CLIPVisionModelHIP
    with pytest.raises(MvdError, match="head dimension"):       # ViT-H/14: 1280 / 16 = 80
        CLIPVisionModelHIP(CLIPVisionConfigLite(hidden_size=1280, num_attention_heads=16, intermediate_size=5120, projection_dim=1024, patch_size=14))
    with pytest.raises(MvdError, match="multiple of patch_size"):
        CLIPVisionModelHIP(CLIPVisionConfigLite(**dict(V.TINY, image_size=30)))
    with pytest.raises(MvdError, match="hidden_act"):
        CLIPVisionModelHIP(CLIPVisionConfigLite(**dict(V.TINY, hidden_act="relu")))
    with pytest.raises(MvdError, match="projection_dim"):
        CLIPVisionModelHIP(CLIPVisionConfigLite(**dict(V.TINY, projection_dim=96)))
    with pytest.raises(MvdError, match="BICUBIC"):
        CLIPImageProcessorLite(resample=2)
    with pytest.raises(MvdError, match="must all be on"):
        CLIPImageProcessorLite(do_center_crop=False)
    p = CLIPImageProcessorLite(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    assert (p.size, p.crop_size) == (32, 32)


# ------------------------------------------------------------------------------- the C ABI on the host
@pytest.fixture(scope="module")
def lib():
    from mvd_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _vcfg(**over):
    from mvd_amd import _lib as L
    c = L.mvd_vision_config_t()
    vals = dict(image_size=32, patch_size=8, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=2, projection_dim=64,
                layer_norm_eps=1e-5, act=1)
    vals.update(over)
    for k, v in vals.items():
        setattr(c, k, v)
    return c


def test_cabi_symbols_exist_and_validate_on_the_host(lib):
    from mvd_amd import _lib as L
    for name in ("mvd_vision_create", "mvd_vision_destroy", "mvd_vision_set_weight", "mvd_vision_workspace_bytes", "mvd_vision_bind_workspace",
                 "mvd_vision_preprocess", "mvd_vision_encode", "mvd_op_clip_pool_project", "mvd_op_clip_cosine"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    h = C.c_void_p()
    for over, msg in ((dict(hidden_size=160, num_heads=2), "head dimension"), (dict(intermediate_size=100), "intermediate_size"),
                      (dict(projection_dim=96), "projection_dim"), (dict(image_size=30), "multiple of patch_size"), (dict(act=2), "act")):
        c = _vcfg(**over)
        assert lib.mvd_vision_create(C.byref(c), C.byref(h)) < 0 and msg in L.last_error(), (over, L.last_error())
    c = _vcfg()
    assert lib.mvd_vision_create(C.byref(c), C.byref(h)) == 0, L.last_error()
    enc1, enc8 = lib.mvd_vision_workspace_bytes(h, 1, 0, 0, 0), lib.mvd_vision_workspace_bytes(h, 8, 0, 0, 0)
    pre8 = lib.mvd_vision_workspace_bytes(h, 8, 768, 768, 32)
    assert 0 < enc1 < enc8 < pre8 < 2 ** 30, (enc1, enc8, pre8)
    assert lib.mvd_vision_workspace_bytes(h, 0, 0, 0, 0) < 0 and "batch" in L.last_error()
    assert lib.mvd_vision_workspace_bytes(h, 1, 5, 0, 32) < 0 and "image size" in L.last_error()
    # nothing below reaches a launch: the arguments, the weight slots and the workspace are checked first
    fake = C.c_void_p(0x10000)
    three = (C.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.mvd_vision_encode(h, fake, 1, None, fake, fake, None) < 0 and "missing weight slot" in L.last_error()
    assert lib.mvd_vision_encode(h, fake, 0, None, fake, fake, None) < 0 and "batch" in L.last_error()
    assert lib.mvd_vision_preprocess(h, fake, 1, 0, 7, 0, 32, 32, three, three, 1, None, None) < 0 and "image size" in L.last_error()
    assert lib.mvd_vision_preprocess(h, fake, 0, 5, 7, 0, 32, 32, three, three, 1, None, None) < 0 and "batch" in L.last_error()
    assert lib.mvd_vision_preprocess(h, fake, 1, 5, 7, 0, 32, 16, three, three, 1, None, None) < 0 and "image_size" in L.last_error()
    assert lib.mvd_vision_preprocess(h, fake, 1, 5, 7, 0, 16, 32, three, three, 1, None, None) < 0 and "smaller than" in L.last_error()
    assert lib.mvd_vision_preprocess(h, fake, 1, 5, 7, 0, 32, 32, three, three, 1, None, None) < 0 and "workspace not bound" in L.last_error()
    assert lib.mvd_vision_bind_workspace(h, C.c_void_p(0x10001), 4096) < 0
    assert lib.mvd_op_clip_cosine(fake, fake, 0, 64, fake, fake, None) < 0
    assert lib.mvd_op_clip_pool_project(fake, None, None, 1, 5, 130, 2, None, None, 1e-5, fake, 64, fake, fake, None) < 0 and "bad shape" in L.last_error()
    assert lib.mvd_op_clip_pool_project(fake, None, None, 1, 5, 128, 2, fake, None, 1e-5, fake, 64, fake, fake, None) < 0 and "go together" in L.last_error()
    lib.mvd_vision_destroy(h)


# ------------------------------------------------------------------------------- CLIPScore on fake snapshots
def test_clip_score_loads_a_snapshot_and_names_each_missing_file(tmp_path):
    from mvd_amd._lib import MvdError
    from mvd_amd.clip_score import FILES, CLIPScore
    snap, parts = build_clip_snapshot(tmp_path / "full")
    m = CLIPScore(snap)
    assert m.model.eos_token_id == 1 and m.processor.size == 32 and m.processor.crop_size == 32 and m.max_length == 77
    assert m.model.vision_model_hip.config.num_tokens == 17 and m.tokenizer.eos_token_id == 1
    assert m._ids(["a photo of a red chair", ""]).tolist() == [[0, 3, 57, 58, 3, 64, 62, 1], [0, 1, 1, 1, 1, 1, 1, 1]]      # padded to the longest
    long = m._ids("chair " * 200)
    assert long.shape == (1, 77) and long[0, -1] == 1          # truncated by the tokenizer: the end token is kept
    assert m.to("cpu") is m
    for name in FILES:
        bad, _ = build_clip_snapshot(tmp_path / ("no_" + name.replace(".", "_")), skip=(name,))
        with pytest.raises(MvdError, match=name.replace(".", r"\.")):
            CLIPScore(bad)
    broken, _ = build_clip_snapshot(tmp_path / "broken")
    open(os.path.join(broken, "model.safetensors"), "wb").write(b"not a safetensors file")
    with pytest.raises(MvdError, match="could not be loaded"):
        CLIPScore(broken)
    with pytest.raises(MvdError, match="no cached snapshot"):
        CLIPScore("fake-org/no-such-clip", cache_dir=str(tmp_path))
    if not torch.cuda.is_available():
        with pytest.raises(MvdError, match="no CPU"):
            m.image_similarity(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))


def test_clip_score_imports_with_transformers_blocked():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('transformers', 'torchmetrics', 'torchvision', 'PIL'):\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            "import mvd_amd.clip_score, mvd_amd.vision_encoder, mvd_amd.validation\n"
            "assert not any(m.split('.')[0] in ('transformers', 'torchmetrics', 'torchvision', 'PIL') for m in sys.modules)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
