"""FID on the GPU (row N10) against tests/fid_ref.py: the convolution kernel on Gaussian inputs under the operator bound of
tests/test_ops_gpu.py, the feature statistics under their accumulation bound, the pool3 features and the FID against the fp32
tower within twice the error of the bf16 emulation (``FEAT_EMU_REL`` / ``FID_EMU_REL``: tests/test_fid_cpu.py measures them),
batch and pass independence bit for bit, torchmetrics' protocol, and ``ValidationScorer`` filling ``fid_score``.

Every figure is for the seeded weights of ``fid_ref.synthetic_inception_state_dict``: the real Inception checkpoint is not
on these machines.  Measured on an MI355X: see DESIGN.md section 9, N10."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import fid_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=1)
def net():
    from mvd_amd.fid import InceptionV3FeaturesHIP
    return InceptionV3FeaturesHIP(R.synthetic_inception_state_dict(0))


@functools.lru_cache(maxsize=1)
def gpu_features():
    """pool3 features of fid_ref.test_images(0) from the GPU, (real, fake): one call each, shared; do not modify"""
    real, fake = R.test_images(0)
    return net()(real.cuda()).cpu(), net()(fake.cuda()).cpu()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("form,B,H,W,cin,cout", [((1, 1, 1, 0, 0), 2, 17, 17, 768, 192), ((1, 7, 1, 0, 3), 2, 17, 17, 160, 192),
                                                 ((3, 3, 2, 0, 0), 1, 35, 35, 288, 384)], ids=["1x1", "1x7", "3x3s2"])
def test_conv_relu_slice_gaussian(form, B, H, W, cin, cout):
    """|err| <= 2^-7 max|ref| (one bf16 ulp of the largest output), the bound of tests/test_ops_gpu.py"""
    from mvd_amd import ops
    from mvd_amd.packing import pack_slice_conv
    kh, kw, stride, ph, pw = form
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(B, H, W, cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, kh, kw, generator=g) / math.sqrt(kh * kw * cin)).to(torch.bfloat16)
    bias = torch.randn(cout, generator=g)
    want = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), bias, stride=stride, padding=(ph, pw))).permute(0, 2, 3, 1)
    for out_f32 in (False, True):
        got = ops.conv_relu_slice(x.cuda(), pack_slice_conv(w).cuda(), bias.cuda(), kh, kw, stride, (ph, pw), out_f32=out_f32).float().cpu()
        err, ref = float((got - want).abs().max()), float(want.abs().max())
        print(f"conv_relu_slice {form} fp32 {out_f32}: max-abs {err:.4g} of {ref:.4g}, rel-L2 {rel(got, want):.3g}")
        assert torch.isfinite(got).all() and err <= 2.0 ** -7 * ref + 1e-6


@pytest.mark.parametrize("n,d", [(5, 64), (8, 2048), (17, 2048)])
def test_feature_stats_gaussian(n, d):
    """per element |err| <= 2 (n + 2) 2^-53 sum_i |f_ia f_ib|: n products and n additions of the accumulation (two calls: the
    second starts from the first's sums) and the final add into the state, each within 2^-53 relative of a partial sum that the
    sum of the absolute products bounds"""
    from mvd_amd import ops
    g = torch.Generator().manual_seed(n + d)
    f1, f2 = torch.randn(n, d, generator=g) + 0.5, torch.randn(n, d, generator=g) * 3
    total = torch.zeros(d, dtype=torch.float64, device="cuda")
    cov = torch.zeros(d, d, dtype=torch.float64, device="cuda")
    ops.feature_stats(f1.cuda(), total, cov)
    ops.feature_stats(f2.cuda(), total, cov)
    f = torch.cat([f1, f2]).double()
    bound = 2 * (2 * n + 2) * 2.0 ** -53
    assert bool(((cov.cpu() - f.t() @ f).abs() <= bound * (f.abs().t() @ f.abs())).all())
    assert bool(((total.cpu() - f.sum(0)).abs() <= bound * f.abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("B,H,W,kind", [(1, 32, 32, "uint8"), (1, 40, 56, "uint8"), (3, 64, 64, "uint8"), (2, 64, 64, "fp32")])
def test_features_against_the_fp32_tower(B, H, W, kind):
    """per-image rel-L2 <= 2 FEAT_EMU_REL: twice the error the number format alone causes"""
    g = torch.Generator().manual_seed(B + H + W)
    smooth = F.interpolate(torch.rand(B, 3, 5, 5, generator=g), size=(H, W), mode="bilinear", align_corners=True)
    x = (smooth * 0.8 + 0.1 + 0.08 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    if kind == "uint8":
        x = (x * 255).round().to(torch.uint8)
    want = R.features(x, 0, False)
    emu = R.features(x, 0, True)
    got = net()(x.cuda()).cpu()
    assert got.shape == (B, 2048) and got.dtype == torch.float32 and torch.isfinite(got).all()
    for i in range(B):
        print(f"features {(B, H, W, kind)} image {i}: GPU vs fp32 tower {rel(got[i], want[i]):.3e}, vs emulation {rel(got[i], emu[i]):.3e}, "
              f"emulation vs fp32 {rel(emu[i], want[i]):.3e} (bound {2 * R.FEAT_EMU_REL:.1e})")
    for i in range(B):
        assert rel(got[i], want[i]) <= 2 * R.FEAT_EMU_REL


def test_features_do_not_depend_on_the_batch_or_the_pass():
    """image i alone == image i inside a batch of 3; two calls give the same bits; 11 images run as passes of 8 + 3 and equal the
    per-image calls"""
    real, fake = R.test_images(0)
    imgs = torch.cat([real, fake, real.flip(3)[:3]]).cuda()      # 11 images
    assert imgs.shape[0] == 11 and net().max_images_per_pass == 8
    all11 = net()(imgs)
    assert torch.equal(all11, net()(imgs))
    batch3 = net()(imgs[:3])
    for i in range(11):
        alone = net()(imgs[i:i + 1])
        assert torch.equal(alone[0], all11[i]), f"image {i} alone differs from image {i} of 11"
        if i < 3:
            assert torch.equal(alone[0], batch3[i]), f"image {i} alone differs from image {i} of 3"
    assert torch.equal(all11[:4].cpu(), gpu_features()[0])


def test_fp32_input_is_quantised():
    real, _ = R.test_images(0)
    as_float = real.float() / 255.0
    assert torch.equal(R.quantise(as_float), real.float())      # k / 255 * 255 truncates back to k for every k
    assert torch.equal(net()(as_float.cuda()).cpu(), gpu_features()[0])
    assert torch.equal(net()((as_float * 3 - 1).cuda()).cpu(), net()((as_float * 3 - 1).clamp(0, 1).cuda()).cpu())


# ------------------------------------------------------------------------------------------------ the metric
def metric(**kw):
    from mvd_amd.fid import FrechetInceptionDistance
    return FrechetInceptionDistance(weights=R.synthetic_inception_state_dict(0), **kw)


def test_fid_fake_against_real():
    real, fake = R.test_images(0)
    m = metric()
    m.update(real.cuda(), real=True)
    m.update(fake.cuda(), real=False)
    got = m.compute()
    assert got.dim() == 0 and got.is_cuda and math.isfinite(float(got))
    g_real, g_fake = gpu_features()
    own, _ = R.fid_of_features(g_real, g_fake)
    print(f"FID {float(got):.9f}; fp64 restatement from the GPU's features {own:.9f}")
    assert abs(float(got) - own) <= 1e-9 * own
    want, _ = R.fid_of_features(*R.reference_features(0, False))
    emu, _ = R.fid_of_features(*R.reference_features(0, True))
    print(f"fp32 tower {want:.6f}, bf16 emulation {emu:.6f}: GPU off by {abs(float(got) - want) / want:.3e}, emulation by {abs(emu - want) / want:.3e} "
          f"(bound {2 * R.FID_EMU_REL:.1e})")
    assert abs(float(got) - want) <= 2 * R.FID_EMU_REL * want
    # the state is what torchmetrics keeps: fp64 sums of the fp32 features, to the accumulation bound
    ref = R.tm_update(R.new_state(), g_real)
    assert int(m.real_features_num_samples) == 4 and m.real_features_sum.dtype == torch.float64
    assert float((m.real_features_sum.cpu() - ref["sum"]).abs().max()) <= 12 * 2.0 ** -53 * float(ref["sum"].abs().max())
    assert float((m.real_features_cov_sum.cpu() - ref["cov_sum"]).abs().max()) <= 12 * 2.0 ** -53 * float(ref["cov_sum"].abs().max())


def test_fid_of_a_set_with_itself():
    real, fake = R.test_images(0)
    both = torch.cat([real, fake]).cuda()
    m = metric()
    m.update(both, real=True)
    m.update(both, real=False)
    assert torch.equal(m.real_features_cov_sum, m.fake_features_cov_sum) and torch.equal(m.real_features_sum, m.fake_features_sum)
    _, tr = R.fid_of_features(torch.cat(gpu_features()), torch.cat(gpu_features()))
    got = float(m.compute())
    print(f"FID of a set with itself {got:.3e}, tr S1 + tr S2 = {tr:.6f}")
    assert abs(got) <= 1e-9 * tr / 2


def test_protocol():
    from mvd_amd._lib import MvdError
    real, fake = R.test_images(0)
    with pytest.raises(ValueError, match="only the 2048"):
        metric(feature=64)
    m = metric(reset_real_features=False).to("cuda")
    for name in m.STATE:
        t = getattr(m, name)
        assert t.is_cuda and t.dtype == (torch.long if name.endswith("num_samples") else torch.float64), name
    assert m.real_features_sum.shape == (2048,) and m.fake_features_cov_sum.shape == (2048, 2048) and m.fake_features_num_samples.dim() == 0
    m.update(real.cuda(), real=True)
    m.update(fake[:1].cuda(), real=False)
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()
    m.update(fake[1:].cuda(), real=False)
    first = float(m.compute())
    kept = m.real_features_cov_sum.clone()
    m.reset()      # reset_real_features=False: the real statistics stay
    assert int(m.fake_features_num_samples) == 0 and int(m.real_features_num_samples) == 4
    assert torch.count_nonzero(m.fake_features_cov_sum) == 0 and torch.count_nonzero(m.fake_features_sum) == 0
    assert torch.equal(m.real_features_cov_sum, kept)
    m.update(fake.cuda(), real=False)
    assert float(m.compute()) == first
    full = metric()
    full.update(real.cuda(), real=True)
    full.reset()
    assert int(full.real_features_num_samples) == 0 and torch.count_nonzero(full.real_features_cov_sum) == 0
    with pytest.raises(MvdError, match="uint8"):
        full.update(real.float().cuda(), real=True)
    with pytest.raises(MvdError, match="floating-point"):
        metric(normalize=True).update(real.cuda(), real=True)


def test_validation_scorer_fills_fid_score():
    """ValidationScorer over the tiny pipeline of tests/test_validation_gpu.py with the stand-in decoder of its fixture: fid_score
    is finite and equals update / update / compute on the decoded images, fed as _fid_score feeds them"""
    from mvd_amd import validation as V
    from mvd_amd.pipeline import MVDPipeline
    from tests import losses_ref as LR
    from tests.parity_util import build_pair, make_inputs
    from tests.test_validation_gpu import _StandinVAE, _scorer_batch, _shifted_acp
    ocfg, params, model = build_pair("tiny", 0, 96, 48)
    inp = make_inputs(ocfg, 3, 16, 7, 0, 96)
    model.fourier_projection = inp["proj"]
    scorer = V.ValidationScorer(MVDPipeline(model, _shifted_acp()), fid_metric_obj=metric(normalize=True))
    scorer.vae = _StandinVAE()
    batch = _scorer_batch(inp)
    ts = torch.tensor([7, 480, 993])
    noise = torch.randn(batch["target_latents"].shape, generator=torch.Generator().manual_seed(5))
    losses = scorer.score(batch, noise=noise, timesteps=ts)
    got = losses["fid_score"]
    assert got.dim() == 0 and got.is_cuda and math.isfinite(float(got)) and float(got) >= 0
    # the same images, directly
    noise_pred, noise_o, noisy, ts_o, target = scorer.forward(batch, noise=noise, timesteps=ts)
    from mvd_amd import ops
    a, s = V.noise_tables(scorer.scheduler, noisy.device)
    _, denoised = ops.noise_loss(noise_pred.float().contiguous(), noise_o, ts_o, a, s, V.snr_table(scorer.scheduler, noisy.device),
                                 scorer.scheduler.config.prediction_type, x0=target, noisy=noisy, snr_gamma=V.SNR_GAMMA, want_denoised=True)
    sf = LR.STANDIN_SCALING_FACTOR
    to01 = lambda z: ((LR.standin_decode(z / sf).float().clamp(-1, 1) + 1) / 2.0).to(torch.float32)      # noqa: E731
    direct = metric(normalize=True)
    direct.update(to01(denoised), real=False)
    direct.update(to01(target), real=True)
    assert float(direct.compute()) == float(got)
