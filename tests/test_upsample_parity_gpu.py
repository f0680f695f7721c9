"""The upsampler convolutions as four 2x2 sub-pixel convolutions of the source map (gemm_pp.hip AMODE 4, packing.pack_up4):
operator level against fp32 torch on the bf16 inputs and the fp32 weights the twin was packed from, and the engine route
(up_blocks.{0,1,2}.up) against the nine-tap route it replaces."""
import math

import pytest
import torch
import torch.nn.functional as F

from mvd_amd._lib import DebugFlag
from tests.test_cfg4_shapes_gpu import _pack, close, grnd      # the bounds of the cfg4 shape tests, exactly as defined there

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def _problem(batch, h, w, cin, cout, seed):
    x = grnd(batch, cin, h, w, seed=seed)
    wt = grnd(cout, cin, 3, 3, scale=1 / math.sqrt(9 * cin), seed=seed + 1, dtype=torch.float32)      # the fp32 master
    bias = grnd(cout, seed=seed + 2, dtype=torch.float32)
    want = F.conv2d(F.interpolate(x.float(), scale_factor=2, mode="nearest"), wt, bias, padding=1).permute(0, 2, 3, 1)
    return x.permute(0, 2, 3, 1).contiguous(), wt, bias, want


def _tiles(batch, h, w, cout):
    return 4 * ((batch * h * w + 255) // 256) * (cout // 320)


@pytest.mark.parametrize("batch,h,w,cin,cout", [
    (32, 32, 32, 640, 640),      # up_blocks.2.up of cfg4: 1024 work items
    (32, 16, 16, 1280, 1280),    # up_blocks.1.up: 512
    (32, 8, 8, 1280, 1280),      # up_blocks.0.up: 128, four images per 256-row tile
    (3, 8, 8, 128, 320),         # rows beyond M inside the only row tile
    (3, 16, 16, 128, 320),       # image borders at tile borders, odd tile count
    (3, 6, 16, 128, 640),        # an image border inside a tile, rows beyond M in the last one
    (2, 48, 48, 128, 320),       # the 48-wide site of 768x768
    (1, 5, 48, 64, 320),         # odd height, M not a multiple of 256
    (3, 16, 16, 64, 320),        # Cin 64: one channel slice, K = 256
])
def test_up4_against_fp32_reference(ops, batch, h, w, cin, cout):
    from mvd_amd.packing import pack_up4
    x, wt, bias, want = _problem(batch, h, w, cin, cout, seed=200)
    w4 = pack_up4(wt)
    got = ops.conv3x3_up4(x, w4, bias)
    plan = ops.last_gemm_plan()
    assert plan["cfg"] == 7 and plan["splitk"] == 1 and plan["tiles"] == _tiles(batch, h, w, cout), plan
    if batch == 32 and h >= 16:
        assert plan["tiles"] > plan["grid"], f"{plan}: every workgroup owned one tile, the cross-tile pipeline did not run"
    what = f"up4 {cin}->{cout} @{batch}x{h}x{w}"
    r = close(got, want, what=what)
    # against the nine-tap kernel on the same data (its weights: the same fp32 master, rounded tap by tap)
    nine = ops.conv3x3(x, _pack(wt), bias, upsample=True)
    d = ((got.float() - nine.float()).norm() / nine.float().norm()).item()
    print(f"{what}: rel-L2 to fp32 {r:.3g}, nine-tap to fp32 {close(nine, want, what='nine-tap'):.3g}, up4 to nine-tap {d:.3g}")
    assert d <= 6e-3, d
    again = ops.conv3x3_up4(x, w4, bias)
    assert torch.equal(got, again), f"{what}: two runs differ"


@pytest.mark.parametrize("h,w", [(12, 12), (24, 24), (7, 8), (16, 20)])
def test_up4_refuses_widths_it_cannot_address(ops, h, w):
    """Source widths whose 16-pixel runs do not map to output rows the same way in every tile come back as an error from the
    operator entry -- never as another kernel, never as a mis-addressed store (the output buffer stays untouched)."""
    from mvd_amd._lib import MvdError
    from mvd_amd.packing import pack_up4
    x, wt, bias, _ = _problem(2, h, w, 128, 320, seed=300)
    before = ops.up4_launches()
    with pytest.raises(MvdError):
        ops.conv3x3_up4(x, pack_up4(wt), bias)
    assert ops.up4_launches() == before


def test_up4_refuses_channel_counts_and_forced_tiles(ops):
    from mvd_amd._lib import MvdError
    from mvd_amd.packing import pack_up4
    x, wt, bias, _ = _problem(2, 16, 16, 128, 256, seed=310)          # N not a multiple of 320
    with pytest.raises(MvdError):
        ops.conv3x3_up4(x, pack_up4(wt), bias)
    x, wt, bias, _ = _problem(2, 16, 16, 128, 320, seed=311)
    with pytest.raises(MvdError):
        ops.conv3x3_up4(x, pack_up4(wt), bias, force_cfg=2)           # the mode exists in the 256x320 ping-pong kernel only


# ------------------------------------------------------------------------------- the engine route
ROUTE_OFF = DebugFlag.NO_UP4      # mvd_debug_set_flags: the upsamplers keep the nine-tap kernel


def _forward(model, inp):
    with torch.no_grad():
        out = model(inp["sample"].cuda(), torch.tensor(500), inp["text"].cuda(), source_camera=inp["src"].cuda(),
                    target_camera=inp["tgt"].cuda(), source_image_latents=inp["lat"].cuda()).sample
    torch.cuda.synchronize()
    return out.float()


def _on_off(batch, hw):
    from mvd_amd import _lib as L, ops as O
    from tests.parity_util import make_inputs, shared_pair
    ocfg, _params, model = shared_pair("sd21")
    inp = make_inputs(ocfg, batch, hw, 77, 0, 1024)
    model.fourier_projection = inp["proj"]
    n0 = O.up4_launches()
    on = _forward(model, inp)
    n_on = O.up4_launches() - n0
    L.lib().mvd_debug_set_flags(ROUTE_OFF)
    try:
        off = _forward(model, inp)
    finally:
        L.lib().mvd_debug_set_flags(0)
    n_off = O.up4_launches() - n0 - n_on
    assert torch.isfinite(on).all() and torch.isfinite(off).all()
    rel = ((on - off).norm() / off.norm()).item()
    print(f"engine, batch {batch}, latent {hw}: sub-pixel route {n_on} launches (off: {n_off}), rel-L2 on vs off {rel:.3g}")
    return n_on, n_off, rel


def test_engine_route_cfg4_shapes():
    """32 pairs at 64x64 latents: the three upsamplers of both passes (main + reference encoder) take the sub-pixel form; with the
    route off none does, and the two forwards agree to the bound of the benchmark's cross-path screen (two correct bf16
    evaluations of this network through different roundings sit about 1e-2 apart)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    n_on, n_off, rel = _on_off(32, 64)
    assert n_on == 6 and n_off == 0, (n_on, n_off)
    assert rel <= 3e-2, rel


def test_engine_keeps_nine_taps_for_widths_the_mode_refuses():
    """96x96 latents (768x768 images), 8 pairs: the 12- and 24-wide upsampler inputs keep the nine-tap launch, the 48-wide one
    takes the sub-pixel form in both passes."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    n_on, n_off, rel = _on_off(8, 96)
    assert n_on == 2 and n_off == 0, (n_on, n_off)
    assert rel <= 3e-2, rel


def test_route_switch_is_read_per_forward_and_leaves_nothing_behind():
    """Setting and clearing a debug switch must leave the product's schedule behind: after NO_UP4 was set and cleared the cfg4-shape
    forward takes the sub-pixel form again (6 launches) and equals, bit for bit, the forward taken before the switch was ever set.
    (1048576 once doubled as the high bit of a launch-policy field whose value stayed on the engine for every later forward.)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import _lib as L, ops as O
    from tests.parity_util import make_inputs, shared_pair
    ocfg, _params, model = shared_pair("sd21")
    inp = make_inputs(ocfg, 32, 64, 77, 0, 1024)
    model.fourier_projection = inp["proj"]
    L.lib().mvd_debug_set_flags(0)
    before = _forward(model, inp)
    n0 = O.up4_launches()
    L.lib().mvd_debug_set_flags(ROUTE_OFF)
    try:
        _forward(model, inp)
    finally:
        L.lib().mvd_debug_set_flags(0)
    n_off = O.up4_launches() - n0
    after = _forward(model, inp)
    n_after = O.up4_launches() - n0 - n_off
    print(f"route off: {n_off} sub-pixel launches, cleared: {n_after}; max |after - before| {(after - before).abs().max().item():.3g}")
    assert n_off == 0 and n_after == 6, (n_off, n_after)
    assert torch.equal(before, after)
