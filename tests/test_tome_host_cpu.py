"""Host logic of token merging, no GPU: argument validation on every surface, which blocks merge at each
``max_downsample``, the ``tome`` config key / ``--tome`` flag of ``mvd_amd.val``, and the C ABI's symbols and host-side refusals."""
from types import SimpleNamespace

import pytest


def _model():
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    return MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", cam_output_dim=96, cam_hidden_dim=48)


def test_enable_tome_on_the_three_surfaces():
    """tomesd's names (ratio, max_downsample) on base_unet (where the reference's users would patch), MultiViewUNet, MVDPipeline"""
    from mvd_amd.pipeline import MVDPipeline
    m = _model()
    assert m.tome is None
    m.base_unet.enable_tome(0.5)
    assert m.tome == (0.5, 1) == m.base_unet.tome
    m.base_unet.disable_tome()
    assert m.tome is None
    m.enable_tome()
    assert m.tome == (0.5, 1)
    m.enable_tome(ratio=0.25, max_downsample=2)
    assert m.tome == (0.25, 2)
    m.disable_tome()
    pipe = MVDPipeline(m, SimpleNamespace(init_noise_sigma=1.0))
    pipe.enable_tome(max_downsample=4, ratio=0.75)
    assert m.tome == (0.75, 4)
    pipe.disable_tome()
    assert m.tome is None and m.base_unet.tome is None


@pytest.mark.parametrize("bad", [(-0.1, 1), (0.76, 1), (float("nan"), 1), (0.5, 0), (0.5, 3), (0.5, 16), (0.5, True)])
def test_enable_tome_validates(bad):
    from mvd_amd.pipeline import MVDPipeline
    m = _model()
    for surface in (m.base_unet, m, MVDPipeline(m, SimpleNamespace(init_noise_sigma=1.0))):
        with pytest.raises(ValueError, match="ratio must lie in|max_downsample must be one of"):
            surface.enable_tome(*bad)
        assert m.tome is None


def test_the_image_encoder_unet_refuses():
    m = _model()
    with pytest.raises(ValueError, match="main pass only"):
        m.image_encoder.unet.enable_tome(0.5)


def test_which_blocks_merge():
    """tomesd's rule ``ceil(sqrt(N0 // N)) <= max_downsample`` on the SD-2.1 topology, with r = min(#src, int(N ratio))"""
    from mvd_amd.config import UNetConfig
    from mvd_amd.unet_params import tome_blocks
    from tests.tome_ref import block_merges
    cfg = UNetConfig.sd21()
    level0 = ["down_block_0_attn_0", "down_block_0_attn_1", "up_block_3_attn_0", "up_block_3_attn_1", "up_block_3_attn_2"]
    level1 = ["down_block_1_attn_0", "down_block_1_attn_1", "up_block_2_attn_0", "up_block_2_attn_1", "up_block_2_attn_2"]
    level2 = ["down_block_2_attn_0", "down_block_2_attn_1", "up_block_1_attn_0", "up_block_1_attn_1", "up_block_1_attn_2"]
    b = tome_blocks(cfg, 64, 64, 0.5, 1)
    assert sorted(b) == sorted(level0) and set(b.values()) == {(64, 64, 2048)}          # the five full-resolution blocks
    b = tome_blocks(cfg, 64, 64, 0.5, 2)
    assert sorted(b) == sorted(level0 + level1) and b["down_block_1_attn_0"] == (32, 32, 512)
    b = tome_blocks(cfg, 64, 64, 0.75, 4)
    assert sorted(b) == sorted(level0 + level1 + level2) and b["up_block_1_attn_2"] == (16, 16, 192) and b["up_block_3_attn_0"] == (64, 64, 3072)
    assert len(tome_blocks(cfg, 64, 64, 0.5, 8)) == 16 and tome_blocks(cfg, 64, 64, 0.5, 8)["mid_block_attn_0"] == (8, 8, 32)
    assert set(tome_blocks(cfg, 96, 96, 0.5, 1).values()) == {(96, 96, 4608)}
    # non-square, odd maps: 48 x 72 latents -> level 2 is 12 x 18, level 3 is 6 x 9 (N0 // N = 64: down = 8)
    b = tome_blocks(cfg, 48, 72, 0.5, 8)
    assert b["mid_block_attn_0"] == (6, 9, 27) and b["down_block_2_attn_1"] == (12, 18, 108)
    # 40 x 56 latents: level 3 is 5 x 7, #src = 35 - 6 = 29, int(35 * 0.75) = 26
    assert tome_blocks(cfg, 40, 56, 0.75, 8)["mid_block_attn_0"] == (5, 7, 26)
    assert tome_blocks(cfg, 64, 64, 0.0, 8) == {}
    # the oracle's rule is the same rule
    for (h, w) in ((64, 64), (96, 96), (48, 72), (40, 56)):
        for mds in (1, 2, 4, 8):
            got = tome_blocks(cfg, h, w, 0.5, mds)
            for lv in range(4):
                H, W = h >> lv, w >> lv
                r = block_merges((h, w), H, W, 0.5, mds)
                names = [n for n, v in got.items() if v[:2] == (H, W)]
                assert (r > 0) == bool(names) and all(got[n][2] == r for n in names), (h, w, mds, lv)


def test_parse_tome():
    from mvd_amd.val import parse_tome
    assert parse_tome(None) is None and parse_tome("") is None
    assert parse_tome("0.5") == (0.5, 1) == parse_tome(0.5) == parse_tome([0.5]) == parse_tome(" 0.5 , 1")
    assert parse_tome("0.25,2") == (0.25, 2) == parse_tome([0.25, 2])
    for bad in ("0.5,1,2", "a", "0.8", "0.5,3", "0.5,1.5", True, [1, 2, 3]):
        with pytest.raises(ValueError):
            parse_tome(bad)


@pytest.mark.parametrize("flag", [None, "0.5", "0.5,2"])
def test_val_flag_reaches_the_config(monkeypatch, tmp_path, flag):
    import mvd_amd.dataset as D
    import mvd_amd.val as V
    seen = {}
    monkeypatch.setattr(V, "load_config", lambda path: dict(image_size=[32, 32], max_views_per_object=4))
    monkeypatch.setattr(V, "setup_pipeline", lambda config, ckpt, device: "pipe")
    monkeypatch.setattr(D, "ObjaverseDataset", lambda **kw: "dataset")
    monkeypatch.setattr(V, "run_validation", lambda pipeline, dataset, config, device, output_dir, **kw: (seen.update(config), ([], {}))[1])
    argv = ["--ckpt", "x.ckpt", "--dataset-path", "data", "--output-dir", str(tmp_path)] + (["--tome", flag] if flag else [])
    assert V.main(argv) == 0
    assert seen.get("tome") == flag
    with pytest.raises(SystemExit):
        V.main(argv[:6] + ["--tome", "0.9"])


def test_run_validation_enables_tome_from_the_config(tmp_path):
    import mvd_amd.val as V
    calls = []

    class Stop(Exception):
        pass

    class Pipe:
        def enable_tome(self, *a):
            calls.append(a)
            raise Stop
    with pytest.raises(Stop):
        V.run_validation(Pipe(), [], dict(batch_size=1, num_workers=0, tome="0.5,2"), "cpu", tmp_path, metrics=object())
    assert calls == [(0.5, 2)]


def test_c_symbols_resolve_and_refuse_on_the_host():
    import ctypes as C
    from mvd_amd import _lib as L
    lib = L.lib()
    for name in ("mvd_op_tome_match", "mvd_op_tome_merge", "mvd_op_tome_unmerge_add", "mvd_op_tome_workspace_bytes", "mvd_debug_tome_plan",
                 "mvd_engine_set_tome", "mvd_engine_clear_tome", "mvd_engine_tome_table"):
        assert getattr(lib, name) is not None
    assert lib.mvd_engine_set_tome(None, 0.5, 1, 0) == -1 and b"null engine" in lib.mvd_last_error()
    assert lib.mvd_engine_clear_tome(None) == -1
    out = (C.c_int64 * 8)()
    assert lib.mvd_debug_tome_plan(64, 64, 320, 2048, out) == 0
    assert list(out) == [1024, 3072, 2048, 4096, 4096, 24, 4096 * 8 + 3072 * 4 + 64, 9216]
    assert lib.mvd_debug_tome_plan(96, 96, 320, 4608, out) == 0 and list(out)[:5] == [2304, 6912, 4608, 8192, 16384]
    assert lib.mvd_debug_tome_plan(96, 97, 320, 10, out) == -1 and b"at most 9216" in lib.mvd_last_error() and out[7] == 9216
    assert lib.mvd_debug_tome_plan(8, 8, 100, 10, out) == -1 and b"multiple of 64" in lib.mvd_last_error()
    assert lib.mvd_debug_tome_plan(8, 8, 64, -1, out) == -1 and b"r = -1" in lib.mvd_last_error()
    assert lib.mvd_op_tome_match(None, 1, 97, 96, 64, 10, None, None, None, None, None, None, 0, None) == -1 and b"at most 9216" in lib.mvd_last_error()
    assert lib.mvd_op_tome_match(None, 1, 8, 8, 64, 10, None, None, None, None, None, None, 0, None) == -1 and b"null tensor" in lib.mvd_last_error()
    assert lib.mvd_op_tome_workspace_bytes(2, 8, 8) == 1024


def test_engine_setting_checks_and_sizing():
    """ratio outside [0, 0.75] and a max_downsample that is no power of two up to 8 are refused by the engine itself, with a
    message; the sizing entries (dry runs, no GPU) take the merging branch: another size, and a map above the select kernel's limit
    is refused there, before anything could be launched"""
    import ctypes as C
    import os

    from mvd_amd import _lib as L
    from mvd_amd.config import UNetConfig
    from tests.test_cabi_cpu import _mk_engine
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.lib()
    rc, h = _mk_engine(lib, UNetConfig.sd21())
    assert rc == 0, L.last_error()
    for ratio, mds in ((-0.01, 1), (0.751, 1), (float("nan"), 1), (0.5, 0), (0.5, 3), (0.5, 16)):
        assert lib.mvd_engine_set_tome(h, ratio, mds, 0) == -1
        assert "set_tome" in L.last_error()
    plain = lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2)
    assert plain > 0, L.last_error()
    assert lib.mvd_engine_set_tome(h, 0.5, 1, 0) == 0, L.last_error()
    merged = lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2)
    assert 0 < merged <= plain, (merged, plain, L.last_error())
    # a block's scratch is released at its end, so the shorter q/k/v buffer LOWERS the peak: at the 8-view guided shape the merging
    # forward needs less than the plain one -- whoever sized a workspace with merging on must size it again once it is off
    plain16 = {}
    for ratio in (0.25, 0.5, 0.75):
        assert lib.mvd_engine_clear_tome(h) == 0
        plain16[ratio] = lib.mvd_engine_workspace_bytes(h, 16, 64, 64, 77, 16)
        assert lib.mvd_engine_set_tome(h, ratio, 1, 0) == 0
        m16 = lib.mvd_engine_workspace_bytes(h, 16, 64, 64, 77, 16)
        assert 0 < m16 < plain16[ratio], (ratio, m16, plain16[ratio], L.last_error())
        assert lib.mvd_engine_clear_tome(h) == 0
        assert lib.mvd_engine_workspace_bytes(h, 16, 64, 64, 77, 16) == plain16[ratio]        # the requirement after clear_tome: the plain one
    assert lib.mvd_engine_set_tome(h, 0.5, 1, 0) == 0
    assert lib.mvd_engine_set_tome(h, 0.5, 1, 1) == 0
    kept = lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2)
    assert kept >= merged + 5 * 2 * 4096 * 4, (kept, merged)                  # five merging blocks keep their [2][4096] int32 tables
    assert lib.mvd_engine_set_tome(h, 0.5, 1, 0) == 0
    assert lib.mvd_engine_workspace_bytes(h, 1, 96, 96, 77, 1) > 0, L.last_error()             # 9216 tokens: the limit itself
    assert lib.mvd_engine_workspace_bytes(h, 1, 96, 104, 77, 1) == -1 and "at most 9216 tokens" in L.last_error()
    assert lib.mvd_engine_set_tome(h, 0.0, 8, 0) == 0
    assert lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2) == plain                          # ratio 0: the forward it always was
    assert lib.mvd_engine_clear_tome(h) == 0
    assert lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2) == plain
    assert lib.mvd_engine_tome_table(h, 0, None, None) == -1 and "not kept" in L.last_error()
    lib.mvd_engine_destroy(h)
