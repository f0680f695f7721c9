"""The transformer tail as one K-concatenated GEMM: ``h' = h + ff.W2^T + b2; out = x + h'.Wp^T + bp`` packed as
``out = x + [ff | h].[Wp.W2 | Wp]^T + (Wp.b2 + bp)`` -- slots ``<key>.tail.w`` / ``.tail.b`` instead of ``ff2`` / ``proj_out``.

Host side only: the composition and its single bf16 rounding, which slots ``pack_unet`` registers with the fold on and off, the
packed bytes, the encoder-weight de-duplication on top of it, and the route the engine's schedule gives the four new GEMM shapes
of a 32-pair forward, of a batch-1 forward and of 96x96 latents (``mvd_debug_dense_route``: host arithmetic, no GPU)."""
import numpy as np
import pytest
import torch

from mvd_amd.config import UNetConfig
from mvd_amd.packing import compose_tail, pack_unet, round_bf16

OLD_SLOTS = ("ff2.w", "ff2.b", "proj_out.w", "proj_out.b")


def _tiny_sd(seed=3):
    from oracle import sd21_unet as OU                     # (test infrastructure: seeded weights of the tiny topology)
    return OU.init_params(OU.UNetConfig.tiny(), seed=seed)


def _nbytes(packed):
    return sum(t.numel() * t.element_size() for t in packed.values())


def _bf16_neighbours(r):
    """the bf16 values next to ``r`` (towards and away from zero), as fp64"""
    bits = r.view(torch.int16).to(torch.int32)
    lo = (bits - 1).to(torch.int16).view(torch.bfloat16).double()
    hi = (bits + 1).to(torch.int16).view(torch.bfloat16).double()
    return lo, hi


def test_round_bf16_rounds_once_to_nearest_even():
    """Values that the fp32 step of torch's fp64 -> bf16 conversion would move exactly onto a bf16 midpoint: the direct rounding goes
    to the neighbour on the value's own side; exact midpoints go to the even neighbour; everything is a nearest bf16 value."""
    base = torch.tensor([1.0, -1.0, 3.140625, -0.0078125, 1.0e-3, 250.0], dtype=torch.bfloat16).double()
    ulp = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -14, 2.0 ** -17, 1.0], dtype=torch.float64)
    eps = ulp * 2.0 ** -30                                   # far below half an fp32 ulp (ulp * 2^-17): the fp32 step lands on the midpoint
    mid = base + torch.sign(base) * ulp / 2                  # (midpoints are exact in fp32 and in fp64)
    above, below = mid + torch.sign(base) * eps, mid - torch.sign(base) * eps
    assert torch.equal(round_bf16(above).double(), base + torch.sign(base) * ulp)
    assert torch.equal(round_bf16(below).double(), base)
    assert torch.equal(round_bf16(mid), mid.float().to(torch.bfloat16))          # ties: to even, as torch does
    # and on random values: no bf16 value is nearer
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g, dtype=torch.float64) * torch.exp(4 * torch.randn(200000, generator=g, dtype=torch.float64))
    r = round_bf16(x)
    lo, hi = _bf16_neighbours(r)
    err = (r.double() - x).abs()
    assert bool(((lo - x).abs() >= err).all()) and bool(((hi - x).abs() >= err).all())


@pytest.mark.parametrize("c", [64, 320])
def test_composition_of_a_random_site(c):
    """``[Wp.W2 | Wp]`` and ``Wp.b2 + bp`` against an independent fp64 evaluation (numpy), and against the two layers applied one
    after the other to random rows."""
    g = torch.Generator().manual_seed(c)
    w2, b2 = torch.randn(c, 4 * c, generator=g) / (4 * c) ** 0.5, torch.randn(c, generator=g)
    wp, bp = torch.randn(c, c, generator=g) / c ** 0.5, torch.randn(c, generator=g)
    w, b = compose_tail(w2, b2, wp, bp)
    assert w.dtype == b.dtype == torch.float64 and tuple(w.shape) == (c, 5 * c) and tuple(b.shape) == (c,)
    w2n, b2n, wpn, bpn = (t.numpy().astype(np.float64) for t in (w2, b2, wp, bp))
    np.testing.assert_allclose(w.numpy(), np.concatenate([wpn @ w2n, wpn], axis=1), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(b.numpy(), wpn @ b2n + bpn, rtol=1e-12, atol=1e-14)
    assert torch.equal(w[:, 4 * c:], wp.double())             # the h columns are proj_out itself
    ff, h, x = (torch.randn(37, k, generator=g, dtype=torch.float64) for k in (4 * c, c, c))
    want = x + (h + ff @ w2.double().T + b2.double()) @ wp.double().T + bp.double()
    got = x + torch.cat([ff, h], 1) @ w.T + b
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_pack_unet_slots_with_the_fold_on_and_off():
    """On (the default): ``tail.w`` [C][5C] bf16 = the fp64 composition of that site's fp32 masters rounded once, ``tail.b`` fp32,
    and none of the slots it replaces.  Off: the old slots, no tail.  Everything else is identical, and the fold does not grow the
    packed bytes."""
    cfg, sd = UNetConfig.tiny(), _tiny_sd()
    on = pack_unet(sd, cfg, "cpu", adapter=False)
    off = pack_unet(sd, cfg, "cpu", adapter=False, fold_tail=False)
    assert set(pack_unet(sd, cfg, "cpu", adapter=False, fold_tail=True)) == set(on)
    sites = cfg.transformers()
    assert sites
    for key, _feat, c, _heads in sites:
        b = f"{key}.transformer_blocks.0"
        w64 = np.concatenate([sd[f"{key}.proj_out.weight"].double().numpy() @ sd[f"{b}.ff.net.2.weight"].double().numpy(),
                              sd[f"{key}.proj_out.weight"].double().numpy()], axis=1)
        b64 = sd[f"{key}.proj_out.weight"].double().numpy() @ sd[f"{b}.ff.net.2.bias"].double().numpy() + sd[f"{key}.proj_out.bias"].double().numpy()
        tw, tb = on[f"{key}.tail.w"], on[f"{key}.tail.b"]
        assert tw.dtype == torch.bfloat16 and tuple(tw.shape) == (c, 5 * c) and tw.is_contiguous()
        assert tb.dtype == torch.float32 and tuple(tb.shape) == (c,)
        # one rounding of the fp64 value: no bf16 value is nearer (the two fp64 products may differ in their last bits)
        x = torch.from_numpy(w64)
        lo, hi = _bf16_neighbours(tw)
        err = (tw.double() - x).abs()
        slack = 1e-12 * x.abs()
        assert bool(((lo - x).abs() + slack >= err).all()) and bool(((hi - x).abs() + slack >= err).all()), key
        np.testing.assert_allclose(tb.numpy(), b64.astype(np.float32), rtol=1e-6, atol=1e-7)
        for s in OLD_SLOTS + ("proj_out.wx",):
            assert f"{key}.{s}" not in on, (key, s)
        assert f"{key}.tail.w" not in off and f"{key}.tail.b" not in off
        for s in OLD_SLOTS:
            assert f"{key}.{s}" in off, (key, s)
        assert off[f"{key}.ff2.w"].numel() + off[f"{key}.proj_out.w"].numel() == tw.numel()
    tail = {k for k in on if ".tail." in k}
    old = {k for k in off if k.endswith(tuple("." + s for s in OLD_SLOTS + ("proj_out.wx",)))}
    assert set(on) - tail == set(off) - old
    for k in set(on) - tail:
        assert torch.equal(on[k], off[k]), k
    assert _nbytes(on) <= _nbytes(off), (_nbytes(on), _nbytes(off))


def test_packed_bytes_do_not_grow_at_the_64x64_level_width():
    """C = 320 is the one width with an X-stationary twin of proj_out (``proj_out.wx``): the fold drops it as well.  One site's
    slots, with the packer's own functions."""
    from mvd_amd.packing import XS_K, pack_xs
    c = XS_K
    g = torch.Generator().manual_seed(5)
    w2, b2 = torch.randn(c, 4 * c, generator=g), torch.randn(c, generator=g)
    wp, bp = torch.randn(c, c, generator=g), torch.randn(c, generator=g)
    w, b = compose_tail(w2, b2, wp, bp)
    new = round_bf16(w).numel() * 2 + b.numel() * 4
    old = (w2.numel() + wp.numel()) * 2 + (b2.numel() + bp.numel()) * 4 + pack_xs(wp, bp).numel() * 2
    assert new < old and round_bf16(w).numel() == w2.numel() + wp.numel()


def test_adapter_and_lean_packing_carry_the_tail_too():
    cfg = UNetConfig.tiny()
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    params = OM.init_mvd_params(OU.UNetConfig.tiny(), 0, cam_dim=96, cam_hidden=48)
    sd = {k[len("base_unet."):]: v for k, v in params.items() if k.startswith("base_unet.")}
    for lean in (False, True):
        packed = pack_unet(sd, cfg, "cpu", adapter=True, ref_scale=0.3, small_batch_twins=not lean)
        for key, _feat, c, _heads in cfg.transformers():
            assert packed[f"{key}.tail.w"].shape == (c, 5 * c) and f"{key}.ff2.w" not in packed and f"{key}.proj_out.w" not in packed


@pytest.mark.parametrize("fold", [True, False])
def test_encoder_weight_dedup_detects_equal_and_differing_weights(monkeypatch, fold):
    """``dedup_encoder_weights="auto"`` compares the two state dicts, not the packed slots: with the fold on or off an image encoder
    that equals the base UNet shares weight set 0, and one whose proj_out -- now part of ``tail.w`` -- differs in ONE element gets
    its own packed set, with its own tail."""
    from mvd_amd import engine as E
    from mvd_amd.mvd_unet import MultiViewUNet
    log = []

    class FakeEngine:
        from mvd_amd.main_options import MainOptions
        options = MainOptions()
        _graph = False

        def __init__(self, *a, device=None, **kw):
            self.device, self.kw = device, kw

        def load_base(self, sd, adapter, ref_scale):
            log.append(("base", set(pack_unet(sd, UNetConfig.tiny(), "cpu", adapter, ref_scale, True, self.kw["fold_tail"]))))

        def load_camera(self, sd):
            pass

        def share_encoder_weights(self, enable=True):
            log.append(("share", enable))

        def load_image_encoder(self, sd):
            log.append(("encoder", pack_unet(sd, UNetConfig.tiny(), "cpu", False, 0.0, True, self.kw["fold_tail"])))

    monkeypatch.setattr(E, "MVDEngine", FakeEngine)
    m = MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", cam_output_dim=96, cam_hidden_dim=48, fold_tail=fold)
    assert m.fold_tail is fold
    monkeypatch.setattr(m, "_exec_device", lambda: torch.device("cpu"))
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(generator=torch.Generator().manual_seed(p.numel()))
        m.image_encoder.unet.load_state_dict({k: v for k, v in m.base_unet.state_dict().items() if ".processor." not in k})
    m._sync_engine()
    assert m.encoder_weights_shared and ("share", True) in log and not any(k == "encoder" for k, _ in log)
    slots = dict(log)["base"]
    key = UNetConfig.tiny().transformers()[0][0]
    assert (f"{key}.tail.w" in slots) == fold and (f"{key}.ff2.w" in slots) == (not fold)
    # one element of one proj_out differs: no sharing, and the encoder's own set is packed the same way
    log.clear()
    with torch.no_grad():
        m.image_encoder.unet.get_parameter(f"{key}.proj_out.weight")[0, 0] += 1.0
    m.mark_weights_changed()
    m._sync_engine()
    assert not m.encoder_weights_shared and ("share", True) not in log
    enc = dict(log)["encoder"]
    assert (f"{key}.tail.w" in enc) == fold and (f"{key}.proj_out.w" in enc) == (not fold)
    assert (f"{key}.tail.w" in dict(log)["base"]) == fold                       # mark_weights_changed re-packs the same slots


# ------------------------------------------------------------------------------------------------ routes of the new shapes
# (family, tile / config, split) by the rules of mvd_gemm_sm_plan, mvd_gemm_pick_config and mvd_gemm_pick_splitk, walked by hand
# for K = 5C.  Tiled configs: 7 = 256x320 ping-pong, 2 = 128x160 lock-step; small-M tile 0 = 64x64.
ROUTES = [
    # 32 pairs, 64x64 latents (cfg4): M = 32 * hw
    (131072, 320, "tiled", 7, 1),      # 512 tiles of 256x320
    (32768, 640, "tiled", 7, 1),       # 256 tiles: one per CU
    (8192, 1280, "tiled", 7, 2),       # 128 tiles, 100 slabs >= 64: the big tile cut in two (50 slabs each; the source boundary is slab 80)
    (2048, 1280, "tiled", 2, 4),       # 128 tiles of 128x160, four slices of 25 slabs (the last one crosses slab 80)
    # 32 pairs, 96x96 latents
    (294912, 320, "tiled", 7, 1),
    (73728, 640, "tiled", 7, 1),
    (18432, 1280, "tiled", 7, 1),      # 288 tiles
    (4608, 1280, "tiled", 2, 1),       # 288 tiles of 128x160 (75 GFLOP: beyond the small-M kernels' 12 GFLOP)
    # batch 1 and 2 (cfg2 / cfg3): the small-M kernels, split where the 64x64 grid is short of 200 tiles
    (4096, 320, "sm", 0, 1),           # 320 tiles
    (1024, 640, "sm", 0, 1),           # 160 tiles: 256 / 160 = 1
    (256, 1280, "sm", 0, 3),           # 80 tiles: 256 / 80 = 3 slices of 33 / 33 / 34 slabs
    (64, 1280, "sm", 0, 8),            # 20 tiles: min(256 / 20, 100 / 12) = 8 slices of 12 / 13 slabs
]


@pytest.mark.parametrize("m,c,family,cfg,splitk", ROUTES)
def test_route_of_the_fused_shapes(m, c, family, cfg, splitk):
    from mvd_amd import ops
    r = ops.engine_dense_route(m, c, 4 * c, c)
    assert r["sm"] == (family == "sm") and r["cfg"] == cfg and r["splitk"] == splitk, r
    assert r["walk_cg"] == 0                       # N = C is 1, 2 or 4 column tiles: the column-group walk starts at 8
    slabs = 5 * c // 64
    assert (4 * c) % 64 == 0 and splitk <= slabs
    if family == "tiled" and splitk > 1:
        assert ops.engine_splitk(m, c, 5 * c) == splitk
    # the one-source launches it replaces keep their routes (ff2: K = 4C)
    old = ops.engine_dense_route(m, c, 4 * c)
    assert old["sm"] == r["sm"]


def test_route_refuses_a_source_that_is_no_multiple_of_the_slab():
    from mvd_amd import _lib as L
    from mvd_amd import ops
    for k1, k2 in ((1280 + 32, 320 - 32), (1280, 96), (100, 0)):
        with pytest.raises(L.MvdError):
            ops.engine_dense_route(2048, 320, k1, k2)
