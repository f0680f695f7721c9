"""FreeU without a GPU: the closed form against diffusers' FFT chain, the wrong variants it must be told
from, the yardstick for the GPU parity bound, and the host surface (three ``enable_freeu`` entries, ``--freeu``, the C symbols)."""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import freeu_ref as FR

# the sizes the closed form was derived for: H = 2 (frequency -1 is the Nyquist frequency), odd sizes, non-squares
SIZES = [(2, 2), (2, 4), (3, 3), (4, 4), (3, 6), (6, 6), (8, 8), (12, 12), (16, 16), (24, 24), (5, 7)]


def _maps(H, W, seed=0, B=2, C=6):
    return torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 131 * H + W))


@pytest.mark.parametrize("s", [0.9, 0.2])
@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_closed_form_is_the_fft_chain(hw, s):
    """(b) == (a) to 2e-6 absolute on N(0, 1) maps: 2e-6 is a few fp32 roundings of the FFT chain (a), which computes in fp32"""
    x = _maps(*hw)
    err = (FR.closed_form(x, s) - FR.fourier_filter(x, 1, s).double()).abs().max().item()
    print(f"closed form vs fft {hw} s={s}: max abs err {err:.3g}")
    assert err <= 2e-6


def test_two_by_two_is_exact():
    """at 2 x 2 every twiddle is +-1 and all four frequencies are masked: skip' = s x, to the last fp32 bit of the FFT chain too"""
    x = _maps(2, 2)
    assert torch.equal(FR.closed_form(x, 0.5), 0.5 * x.double())
    assert (FR.fourier_filter(x, 1, 0.5) - 0.5 * x).abs().max().item() <= 1e-7


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("hw", [(4, 4), (4, 8), (6, 6), (8, 8), (16, 16), (5, 7)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_wrong_variants_are_far(hw):
    """the three faults a kernel could have are at least 1e-2 of the norm away at s = 0.2 on maps with H, W >= 4"""
    x = _maps(*hw)
    want = FR.fourier_filter(x, 1, 0.2)
    d = dict(flip=_rel(FR.closed_form(x, 0.2, flip_one_axis=True), want), no_dc=_rel(FR.closed_form(x, 0.2, drop_dc=True), want),
             upper_half=_rel(FR.backbone_scale(x, 1.4, upper_half=True), FR.apply_freeu(0, x, x, **FR.SD21)[0]))
    print(f"wrong variants {hw}: {d}")
    assert min(d.values()) >= 1e-2, d


@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 2), (2, 7)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_flipped_mode_is_the_same_function_on_two_rows_or_columns(hw):
    """with H or W = 2 the flipped (1, 1) mode is the right one (-1 = +1 on that axis): no test can tell them apart there"""
    x = _maps(*hw)
    assert (FR.closed_form(x, 0.2, flip_one_axis=True) - FR.closed_form(x, 0.2)).abs().max().item() <= 1e-12


def test_apply_freeu_touches_blocks_0_and_1_only():
    h, sk = _maps(4, 4, 1), _maps(4, 4, 2)
    h2, sk2 = FR.apply_freeu(2, h, sk, **FR.SD21)
    assert h2 is h and sk2 is sk
    h0, _ = FR.apply_freeu(0, h, sk, **FR.SD21)
    h1, _ = FR.apply_freeu(1, h, sk, **FR.SD21)
    assert torch.equal(h0[:, :3], h[:, :3] * 1.4) and torch.equal(h1[:, :3], h[:, :3] * 1.6) and torch.equal(h0[:, 3:], h[:, 3:])


# ---------------------------------------------------------------------------------------------- the yardstick of the GPU bounds
@functools.lru_cache(maxsize=None)
def _yardstick(hw, setting):
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs, rel_l2
    cfg = OU.UNetConfig.tiny()
    params = OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)
    inp = make_inputs(cfg, 2, hw, 7, 0, 96)
    kw = dict(setting)

    def fwd():
        return OM.multiview_unet_forward(params, cfg, inp["sample"], torch.tensor(500), inp["text"], inp["src"], inp["tgt"], inp["lat"],
                                         fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)
    plain = fwd()
    with FR.freeu_oracle(**kw):
        want = fwd()
    d = dict(plain=rel_l2(plain, want))
    variants = dict(blocks012=dict(blocks=(0, 1, 2)), b_only=dict(use_s=False), s_only=dict(use_b=False))
    if hw != 16:
        variants["flip"] = dict(flip_one_axis=True)           # (16 x 16 latents: the maps are 2 x 2 and 4 x 4)
    for name, v in variants.items():
        with FR.freeu_oracle(**kw, **v):
            d[name] = rel_l2(fwd(), want)
    swapped = dict(s1=kw["s2"], s2=kw["s1"], b1=kw["b2"], b2=kw["b1"])
    with FR.freeu_oracle(**swapped):
        d["swapped"] = rel_l2(fwd(), want)
    return d


@pytest.mark.parametrize("hw", [16, (16, 32)], ids=["16x16", "16x32"])
def test_parity_setting_tells_every_wrong_function_apart(hw):
    """Tiny topology, batch 2, img_ref_scale 0.3: the FreeU oracle forward under the PARITY setting is at least four times the GPU
    parity bound away from the plain forward, from FreeU on blocks 0-2, from b only, from s only, from the one-axis-flipped (1, 1)
    mode (16 x 32) and from the two blocks' values swapped -- so the engine parity test cannot pass on any of them.

    Measured (rel-L2), PARITY_SETTING s1=16 s2=24 b1=2 b2=2.5:
      16 x 16: plain 0.499, blocks 0-2 0.926, b only 0.485, s only 0.332, swapped 0.222
      16 x 32: plain 0.555, blocks 0-2 0.958, b only 0.541, s only 0.375, flipped 0.143, swapped 0.264
    The published SD-2.1 setting (s1=0.9 s2=0.2 b1=1.4 b2=1.6) gives plain 0.081 / 0.075, b only 0.074 / 0.058, s only 0.050 / 0.056,
    flipped 0.020 at 16 x 32: below four times any bound near 2e-2, which is why the parity tests use the stronger setting (the
    SD-2.1 setting is compared as well, under the same bound)."""
    d = _yardstick(hw, tuple(sorted(FR.PARITY_SETTING.items())))
    print(f"yardstick {hw} {FR.PARITY_SETTING}: {d}")
    assert min(d.values()) >= 4 * FR.PARITY_BOUND_MAX, d


def test_sd21_setting_yardstick_is_recorded():
    """the published setting's own distances (printed for DESIGN.md; the only assertion is that FreeU does something)"""
    d = _yardstick((16, 32), tuple(sorted(FR.SD21.items())))
    print(f"yardstick (16, 32) {FR.SD21}: {d}")
    assert d["plain"] > 2 * FR.PARITY_BOUND_MAX


def test_freeu_oracle_leaves_the_encoder_pass_alone():
    """the oracle's encoder pass (the forward with ``capture``) is the same with and without the context"""
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    cfg = OU.UNetConfig.tiny()
    p = OU.init_params(cfg, 3)
    g = torch.Generator().manual_seed(5)
    lat, text = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 7, cfg.cross_attention_dim, generator=g)
    plain = OM.image_encoder_forward(p, cfg, lat, text)
    with FR.freeu_oracle(**FR.PARITY_SETTING):
        inside = OM.image_encoder_forward(p, cfg, lat, text)
        main = OU.unet_forward(p, cfg, lat, torch.tensor([0]), text)
    assert all(torch.equal(plain[k], inside[k]) for k in plain)
    assert not torch.equal(main, OU.unet_forward(p, cfg, lat, torch.tensor([0]), text))
    assert OU.unet_forward.__module__ == "oracle.sd21_unet" and OU.resnet_block.__module__ == "oracle.sd21_unet"      # put back


# ---------------------------------------------------------------------------------------------- host surface
def _model():
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    return MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", cam_output_dim=96, cam_hidden_dim=48)


def test_enable_freeu_on_the_three_surfaces():
    """diffusers' argument order (s1, s2, b1, b2) and names, on base_unet (the reference's call site), MultiViewUNet, MVDPipeline"""
    from mvd_amd.pipeline import MVDPipeline
    m = _model()
    assert m.freeu is None
    m.base_unet.enable_freeu(0.9, 0.2, 1.4, 1.6)
    assert m.freeu == (0.9, 0.2, 1.4, 1.6) == m.base_unet.freeu
    m.base_unet.disable_freeu()
    assert m.freeu is None
    m.enable_freeu(s1=0.9, s2=0.2, b1=1.4, b2=1.6)
    assert m.freeu == (0.9, 0.2, 1.4, 1.6)
    m.disable_freeu()
    assert m.freeu is None
    pipe = MVDPipeline(m, SimpleNamespace(init_noise_sigma=1.0))
    pipe.enable_freeu(b2=1.6, b1=1.4, s2=0.2, s1=0.9)
    assert m.freeu == (0.9, 0.2, 1.4, 1.6)
    pipe.disable_freeu()
    assert m.freeu is None and m.base_unet.freeu is None


@pytest.mark.parametrize("bad", [(0.0, 0.2, 1.4, 1.6), (0.9, -0.2, 1.4, 1.6), (0.9, 0.2, float("nan"), 1.6), (0.9, 0.2, 1.4, float("inf"))])
def test_enable_freeu_validates(bad):
    from mvd_amd.pipeline import MVDPipeline
    m = _model()
    for surface in (m.base_unet, m, MVDPipeline(m, SimpleNamespace(init_noise_sigma=1.0))):
        with pytest.raises(ValueError, match="positive and finite"):
            surface.enable_freeu(*bad)
        assert m.freeu is None
    with pytest.raises(TypeError):
        m.enable_freeu(0.9, 0.2, 1.4)


def test_the_image_encoder_unet_refuses():
    """FreeU on the encoder pass is not a thing (the reference's ImageEncoder owns a UNet nobody enables it on)"""
    m = _model()
    with pytest.raises(ValueError, match="main pass only"):
        m.image_encoder.unet.enable_freeu(0.9, 0.2, 1.4, 1.6)


def test_parse_freeu():
    from mvd_amd.val import parse_freeu
    assert parse_freeu(None) is None and parse_freeu("") is None
    assert parse_freeu("0.9,0.2,1.4,1.6") == (0.9, 0.2, 1.4, 1.6) == parse_freeu([0.9, 0.2, 1.4, 1.6]) == parse_freeu(" 0.9, 0.2 ,1.4,1.6")
    for bad in ("0.9,0.2,1.4", "0.9,0.2,1.4,1.6,2", "a,b,c,d", "0.9,0.2,1.4,0", [1, 2, 3]):
        with pytest.raises(ValueError):
            parse_freeu(bad)


@pytest.mark.parametrize("flag", [None, "0.9,0.2,1.4,1.6"])
def test_val_flag_reaches_the_pipeline(monkeypatch, tmp_path, flag):
    """``--freeu`` through ``main`` lands in the config; ``run_validation`` enables it on the pipeline, and only when the key is there"""
    import mvd_amd.dataset as D
    import mvd_amd.val as V
    seen = {}
    monkeypatch.setattr(V, "load_config", lambda path: dict(image_size=[32, 32], max_views_per_object=4))
    monkeypatch.setattr(V, "setup_pipeline", lambda config, ckpt, device: "pipe")
    monkeypatch.setattr(D, "ObjaverseDataset", lambda **kw: "dataset")
    monkeypatch.setattr(V, "run_validation", lambda pipeline, dataset, config, device, output_dir, **kw: (seen.update(config), ([], {}))[1])
    argv = ["--ckpt", "x.ckpt", "--dataset-path", "data", "--output-dir", str(tmp_path)] + (["--freeu", flag] if flag else [])
    assert V.main(argv) == 0
    assert seen.get("freeu") == flag
    with pytest.raises(SystemExit):
        V.main(argv[:6] + ["--freeu", "0.9,0.2"])


def test_run_validation_enables_freeu_from_the_config(tmp_path):
    import mvd_amd.val as V
    calls = []

    class Stop(Exception):
        pass

    class Pipe:
        def enable_freeu(self, *a):
            calls.append(a)
            raise Stop
    cfg = dict(batch_size=1, num_workers=0, freeu="0.9,0.2,1.4,1.6")
    with pytest.raises(Stop):
        V.run_validation(Pipe(), [], cfg, "cpu", tmp_path, metrics=object())
    assert calls == [(0.9, 0.2, 1.4, 1.6)]


def test_c_symbols_resolve():
    from mvd_amd import _lib as L
    lib = L.lib()
    for name in ("mvd_op_freeu", "mvd_engine_set_freeu", "mvd_engine_clear_freeu"):
        assert getattr(lib, name) is not None
    # null engine / bad values are answered on the host, without a GPU
    assert lib.mvd_engine_set_freeu(None, 0.9, 0.2, 1.4, 1.6) == -1 and b"null engine" in lib.mvd_last_error()
    assert lib.mvd_engine_clear_freeu(None) == -1
    assert lib.mvd_op_freeu(None, 8, None, 8, 1, 2, 2, 1.0, 1.0, None, None, None) == -1 and b"null tensor" in lib.mvd_last_error()
