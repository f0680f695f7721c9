"""The float64 references of tests/conditioning_ref.py pinned to the oracle (oracle/mvd.py, oracle/sd21_unet.py -- themselves
pinned to the reference project's golden vectors), and the CPU side of every bound tests/test_conditioning_ops_gpu.py holds the
kernels to: each bound is derived here, from the references and from float32 emulations of the kernels' formulas, without a GPU."""
import pytest
import torch

from oracle import mvd as OM
from oracle import sd21_unet as OU
from tests import conditioning_ref as CR


# ------------------------------------------------------------------------------------------------ pinned to the oracle
@pytest.mark.parametrize("dim", CR.TIMESTEP_DIMS)
def test_timestep_embedding_matches_oracle(dim):
    t = torch.tensor(CR.TIMESTEP_VALUES)
    want, ang, arg = CR.timestep_embedding(t, dim)
    got = OU.timestep_embedding(t, dim)
    assert got.shape == want.shape
    assert ((got.double() - want).abs() <= CR.timestep_embedding_bound(ang, arg)).all()
    half = dim // 2
    assert torch.equal(want[:, :half], torch.cos(ang)) and torch.equal(want[:, half:], torch.sin(ang))   # [cos | sin]


@pytest.mark.parametrize("rows", [3, 4])
def test_relative_transform_and_fourier_features_match_oracle(rows):
    src, tgt = CR.random_cameras(5, rows, seed=rows)
    R, T = CR.relative_transform(src, tgt)
    oR, oT = OM.relative_transform(src, tgt)
    torch.testing.assert_close(oR.double(), R, rtol=0, atol=2e-6)
    torch.testing.assert_close(oT.double(), T, rtol=0, atol=4e-6)
    # the oracle's layout is the kernel's: per axis [sin nfreq | cos nfreq]; fed the float64 T rounded to fp32, so that only the
    # feature formula is compared
    for out_dim in (12, 96, 1020):
        nfreq = (out_dim // 2) // 3
        cf = CR.camera_features(src, tgt, nfreq)
        got = OM.fourier_features(T.float(), out_dim)
        assert got.shape == cf["enc"].shape
        assert ((got.double() - cf["enc"]).abs() <= CR.camera_features_bound(cf["ang"], cf["arg"])).all(), out_dim


def test_non_orthonormal_cameras_tell_the_orders_apart():
    """the test cameras make a transpose or an order mistake a first-order error (orthonormal ones can hide sR tR^T)"""
    src, tgt = CR.random_cameras(5, 4, seed=1)
    R, _ = CR.relative_transform(src, tgt)
    s, g = src.double()[:, :3, :3], tgt.double()[:, :3, :3]
    for wrong in (s @ g.transpose(1, 2), g @ s, g.transpose(1, 2) @ s):
        assert (wrong - R).abs().max() > 0.5


@pytest.mark.parametrize("simple", [False, True])
def test_camera_embedding_and_film_match_oracle(simple):
    cfg = CR.small_cfg()
    p = OM.init_camera_params(cfg, 3, 96, 48, simple)
    g = torch.Generator().manual_seed(2)
    proj = OM.draw_fourier_projection(96, g)
    src, tgt = CR.random_cameras(4, 4, seed=7)
    want = CR.camera_embedding(p, src, tgt, proj, simple)
    got = OM.camera_embedding(p, src, tgt, proj, simple)
    torch.testing.assert_close(got.double(), want, rtol=0, atol=2e-5)
    for name in OM.modulation_hidden_dims(cfg):
        sc, sh = CR.modulator_film(p, name, want, 0.5)
        osc, osh = OM.film_scale_shift(p, name, want.float(), 0.5)
        torch.testing.assert_close(osc.double(), sc, rtol=0, atol=2e-6)
        torch.testing.assert_close(osh.double(), sh, rtol=0, atol=2e-6)


def test_time_projection_reference_matches_oracle_steps():
    """the float64 time projection with fp32 weights equals the oracle's own steps at fp32 agreement, and its slices follow the
    module order of the oracle's parameter names"""
    cfg = OU.UNetConfig.tiny()
    p = OU.init_params(cfg, 0)
    keys = CR.resnet_keys(p.keys())
    assert keys[0] == "down_blocks.0.resnets.0" and keys[-1].startswith("up_blocks.3.resnets.")
    assert keys.index("mid_block.resnets.0") == cfg.num_levels * cfg.layers_per_block
    assert len(keys) == len([k for k in p if k.endswith("time_emb_proj.bias")])
    t = torch.tensor([0.0, 321.0, 999.0])
    f32 = CR.time_projection_f32(p, t, cfg.block_out_channels[0])
    # bf16 storage is the engine's choice, not the oracle's: compare the fp32-weight oracle at bf16-storage agreement ...
    want = CR.time_projection(p, t, cfg.block_out_channels[0])
    for i in want:
        assert f32[i].shape == want[i].shape
        assert (f32[i].double() - want[i]).abs().max() <= 2e-2 * max(1.0, want[i].abs().max().item())
    # ... and at fp32 agreement once the same bf16-rounded weights are given to both
    pb = {k: (v.to(torch.bfloat16).float() if k.endswith(".weight") and v.dim() == 2 else v) for k, v in p.items()}
    f32b, wantb = CR.time_projection_f32(pb, t, cfg.block_out_channels[0]), CR.time_projection(pb, t, cfg.block_out_channels[0])
    for i in wantb:       # (the reference rounds SiLU(emb) to bf16: 2^-9 relative on a K = 256 sum of O(1/16) weights)
        assert (f32b[i].double() - wantb[i]).abs().max() <= 2.0 ** -8 * max(1.0, wantb[i].abs().max().item())


# ------------------------------------------------------------------------------------------------ bounds, derived on the CPU
def test_sinusoid_bound_holds_a_float32_emulation_with_margin():
    """The kernels' formulas step by step in numpy float32 stay at or below 0.45 of |ang| (3 + |arg|) 2^-23 + 2^-23 on every case
    of the GPU tests (measured: 0.43 at worst for the timestep embedding)."""
    worst = 0.0
    for dim in CR.TIMESTEP_DIMS:
        for batch in (1, 3):
            for k in range(len(CR.TIMESTEP_VALUES)):
                t = torch.tensor([CR.TIMESTEP_VALUES[(k + j) % len(CR.TIMESTEP_VALUES)] for j in range(batch)])
                want, ang, arg = CR.timestep_embedding(t, dim)
                emu = CR.timestep_embedding_f32(t.numpy(), dim)
                worst = max(worst, ((emu.double() - want).abs() / CR.timestep_embedding_bound(ang, arg)).max().item())
    print(f"timestep embedding: worst float32-emulation error / bound = {worst:.3f}")
    assert worst <= 0.45, worst
    worst_c = 0.0
    for nfreq in CR.CAMERA_NFREQ:
        for batch in (1, 5):
            for rows in (3, 4):
                src, tgt = CR.random_cameras(batch, rows, seed=batch, grid=True)
                cf = CR.camera_features(src, tgt, nfreq)
                rflat, enc = CR.camera_features_f32(src.numpy(), tgt.numpy(), nfreq)
                worst_c = max(worst_c, ((enc.double() - cf["enc"]).abs() / CR.camera_features_bound(cf["ang"], cf["arg"])).max().item())
                assert torch.equal(rflat.double(), cf["rflat"]) and torch.equal(cf["T"].float().double(), cf["T"])   # exact inputs
                # full-precision entries: R within 4 ulp of the sum of its terms' magnitudes
                src, tgt = CR.random_cameras(batch, rows, seed=batch)
                cf = CR.camera_features(src, tgt, nfreq)
                rflat, _ = CR.camera_features_f32(src.numpy(), tgt.numpy(), nfreq)
                assert ((rflat.double() - cf["rflat"]).abs() <= CR.rflat_bound(cf["rflat_mag"])).all()
    print(f"camera features: worst float32-emulation error / bound = {worst_c:.3f}")
    assert worst_c <= 0.45, worst_c


@pytest.mark.parametrize("c,rows,silu", CR.LN_CASES)
def test_layernorm_bound_is_positive_and_small(c, rows, silu):
    x, gamma, beta = CR.ln_case(c, rows, silu)
    b = CR.layernorm_bound(x, gamma, beta, 1e-5, silu)
    assert 0.0 < b < 2e-5, b


def test_layernorm_probe_discriminates_the_one_pass_variance():
    """rows of mean 100, deviation 0.1: the two-pass emulation's error sets the bound; E[x^2] - mean^2 in fp32 misses it"""
    x = CR.layernorm_probe()
    c = x.shape[1]
    gamma, beta = torch.ones(c), torch.zeros(c)
    want = CR.layernorm_f32(x, gamma, beta)
    bound = CR.layernorm_bound(x, gamma, beta)
    one = CR.layernorm_f32_emulated(x.numpy(), gamma.numpy(), beta.numpy(), one_pass=True)
    bad = (one.double() - want).abs()
    bad = torch.where(torch.isfinite(bad), bad, torch.full_like(bad, float("inf"))).max().item()
    print(f"mean-100 probe: bound {bound:.3e}, one-pass variance error {bad:.3e}")
    assert bound < 1e-2 and bad > bound, (bound, bad)


def test_grouped_layernorm_reference_uses_one_affine_per_segment():
    x, gamma, beta = CR.ln_case(48, 27, True, nseg=9)
    want = CR.layernorm_f32(x, gamma, beta, 1e-5, True, 9)
    for r in (0, 8, 9, 26):
        alone = CR.layernorm_f32(x[r:r + 1], gamma[r % 9], beta[r % 9], 1e-5, True)
        assert torch.equal(alone[0], want[r])
    wrong = CR.layernorm_f32(x, gamma.roll(1, 0), beta.roll(1, 0), 1e-5, True, 9)
    assert (wrong - want).abs().max() > 0.05          # every segment's affine differs from its neighbour's at O(0.1)


def test_grouped_linear_reference_reads_its_own_segment():
    g = torch.Generator().manual_seed(3)
    seg = [6, 70, 78]
    x, w = torch.randn(4, 3 * 48, generator=g), torch.randn(78, 48, generator=g)
    want = CR.linear_grouped(x, w, seg)
    assert torch.equal(want[:, 6:70], x.double()[:, 48:96] @ w.double()[6:70].T)
    assert (CR.linear_grouped(x.roll(48, 1), w, seg) - want).abs().max() > 1.0     # the neighbour's segment is wrong by O(1)


def test_film_params_reference_saturates_and_cycles():
    raw = torch.tensor([[100.0, -100.0, 0.0, 3.0, -2.0, 0.5], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    sc, sh = CR.film_params(raw, 0.2, out_rows=4)
    assert sc[0, 0] == 0.4 and abs(sc[0, 1].item()) < 1e-40 and sc[0, 2] == 0.2 and torch.equal(sh[0], 0.2 * raw[0, 3:].double())
    assert torch.equal(sc[2], sc[0]) and torch.equal(sc[3], sc[1]) and torch.equal(sh[3], sh[1])
    flat = CR.grouped_layout(CR.film_params_grouped(raw, [2, 6], 1.0, out_rows=3))
    assert flat.numel() == 3 * 6
    assert torch.equal(flat[:3], 2 * torch.sigmoid(raw.double()[[0, 1, 0], 0]))            # segment 0 (dim 1): scale rows
    assert torch.equal(flat[6:12].view(3, 2), 2 * torch.sigmoid(raw.double()[[0, 1, 0], 2:4]))   # segment 1 starts at rows * 2


@pytest.mark.parametrize("C", [1, 3, 4, 7])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 8)])
def test_im2col_reference_and_film_rounding_share(C, hw):
    h, w = hw
    from tests.exact_util import round_f64_to_bf16
    g = torch.Generator().manual_seed(C * 100 + h * 10 + w)
    x = torch.randn(2, C, h, w, generator=g)
    val, inside = CR.im2col_in(x)
    assert not inside[..., 9 * C:].any() and (val[~inside] == 0).all()
    assert torch.equal(val[:, :, :, 4 * C:5 * C], x.double().permute(0, 2, 3, 1))            # the centre tap is the pixel itself
    if h > 1:
        assert torch.equal(val[:, 1:, :, 1 * C:2 * C], x.double().permute(0, 2, 3, 1)[:, :-1])  # tap 1 = the pixel above
        assert not inside[:, 0, :, :3 * C].any()
    # FiLM: neither fp32 form (one fma, or a multiply then an add) moves more than 1 % of the elements off the float64 result's
    # bf16 rounding, and none by more than one bf16 ulp
    from tests.exact_util import ulp_distance
    for ld_ss in (0, 4, 8):
        xf, scale, shift = CR.im2col_film_case(C, h, w, ld_ss)
        want64, ins = CR.im2col_in(xf, scale, shift, ld_ss)
        want = round_f64_to_bf16(want64)
        for fma in (True, False):
            v32, _ = CR.im2col_in(CR.im2col_film_f32(xf, scale, shift, ld_ss, fma))
            got = v32.float().to(torch.bfloat16)
            dist = ulp_distance(got, want)
            assert dist.max() <= 1 and (dist[ins] != 0).double().mean() < 0.01, (C, hw, ld_ss, fma)


def test_embedding_film_and_time_bounds_are_derived_from_the_fp32_oracle():
    """8 x the worst difference between the float32 torch oracle and the float64 reference: the figures the GPU tests use
    (conditioning_bounds()), printed."""
    b = CR.conditioning_bounds()
    print({k: f"{v:.3e}" for k, v in b.items()})
    assert 0 < b["embedding"] < 1e-4 and 0 < b["film"] < 1e-4 and 0 < b["time"] < 1e-3, b
    # the time bound's two stages: few activations sit near enough to a bf16 tie to be allowed a one-ulp store difference
    pb, c0, ts = CR.time_case()
    for t in ts:
        bounds, f = CR.time_bound(pb, t, c0)
        print(f)
        # (t = 999 carries |ang| 2^-23 ~ 1e-4 of angle error into the sinusoid in ANY fp32 evaluation: stage A is not tight, and
        #  a fifth of that row's stored activations may round either way.  The bound stays far below a slice in the wrong place,
        #  whose error is the size of the outputs, 0.1 to 1.)
        assert f["near_ties"] <= 0.25 * f["activations"] and all((b > 0).all() for b in bounds.values())
        assert max(b.max().item() for b in bounds.values()) < 5e-3
