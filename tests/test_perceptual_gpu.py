"""The VGG-16 perceptual loss on the MI355X: ``mvd_vgg_features`` / ``mvd_vgg_perceptual`` and the Python
surface over them against the fp32 restatement of tests/vgg_ref.py, with the synthetic weights and images defined there.

Bounds (none comes from what the kernels give):
* features and the four taps: rel-L2 against the fp32 tower <= 2 x the rel-L2 of the bf16-storage emulation at that tap, computed
  here on the CPU (4.9e-3 - 5.4e-3 at conv5_3).  The emulation differs from the GPU path in accumulation order only; the factor
  2 covers that;
* the squared-difference kernels: against ``F.mse_loss`` of the GPU's own features in fp64, <= 1e-5 relative (the sums run in
  fp64: what is left is one fp32 rounding of the result, 6e-8);
* the loss against the fp32 tower: with f the true maps and e the feature bound above, E = e (rms fx + rms fy) bounds the rms
  error of fx - fy, so |dL| <= 2 sqrt(L) E + E^2;
* per-sample values: each within that bound of the single-pair call; their mean against the batch loss <= 1e-6 relative (both are
  fp64 sums of the same per-pair sums; the per-pair values are rounded to fp32 once, 6e-8 each, and so is the batch loss).
Shapes are pairs x H x W of vgg_ref.SHAPES: odd pool sizes (40 x 56: 5 x 7 -> 2 x 3), passes of 2 + 1 pairs, M below one tile."""
import pytest
import torch
import torch.nn.functional as F

import vgg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def loss_fn():
    from mvd_amd.perceptual import PerceptualLoss
    return PerceptualLoss("cuda", weights=R.synthetic_state_dict())


def make_loss(pairs):
    """the third shape runs in passes of 2 + 1 pairs"""
    from mvd_amd.perceptual import PerceptualLoss
    return PerceptualLoss("cuda", weights=R.synthetic_state_dict(), max_pairs_per_pass=2 if pairs == 3 else 8)


def loss_bound(eps, fx, fy):
    L = F.mse_loss(fx.double(), fy.double()).item()
    E = eps * (R.rms(fx) + R.rms(fy))
    return L, 2 * L ** 0.5 * E + E * E


@pytest.mark.parametrize("pairs,h,w", R.SHAPES)
def test_features_and_taps(pairs, h, w):
    from mvd_amd.perceptual import TAP_NAMES, VGG16FeaturesHIP
    c = R.case(pairs, h, w)
    m = VGG16FeaturesHIP()
    m.load_state_dict(c.sd)
    both = torch.cat([c.x, c.y]).cuda()
    feat, taps = m(both, taps=True)
    assert feat.shape == c.feat.shape and feat.dtype == torch.float32 and list(taps) == list(TAP_NAMES)
    assert feat.permute(0, 2, 3, 1).is_contiguous()                      # an NCHW view of the NHWC buffer
    for name, want in list(c.taps.items()) + [("conv5_3", c.feat)]:
        got = feat if name == "conv5_3" else taps[name]
        assert got.shape == want.shape, name
        err = R.rel_l2(got.float().cpu(), want)
        print(f"{(pairs, h, w)} {name}: GPU rel-L2 {err:.3e}, emulation {c.emu[name]:.3e}, bound {2 * c.emu[name]:.3e}")
        assert err <= 2 * c.emu[name], (name, err, c.emu[name])
    # without the taps: the same features, bit for bit (the taps only redirect where four maps are written)
    assert torch.equal(m(both), feat)


@pytest.mark.parametrize("close", [False, True], ids=["independent", "close"])
@pytest.mark.parametrize("pairs,h,w", R.SHAPES)
def test_loss_against_the_fp32_tower(pairs, h, w, close):
    c = R.case(pairs, h, w, close)
    loss = make_loss(pairs)
    got = loss(c.x.cuda(), c.y.cuda())
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
    L, bound = loss_bound(2 * c.emu["conv5_3"], c.feat[:pairs], c.feat[pairs:])
    print(f"{(pairs, h, w)} close={close}: GPU loss {got.item():.6e}, fp32 tower {L:.6e}, |dL| {abs(got.item() - L):.3e}, bound {bound:.3e}")
    assert abs(got.item() - L) <= bound
    if not close:
        # the squared-difference kernels alone: the loss against the GPU's own features.  They are asked for pass by pass, as
        # [x of the pass; y of the pass]: the split-K choice of a convolution depends on the batch, a different split moves fp32 sums
        # by an ulp, and an ulp flips bf16 roundings of the stored maps (1e-4 of the loss: the tower's tolerance, not this one's)
        pp = loss.max_pairs_per_pass
        fx, fy = [], []
        for p0 in range(0, pairs, pp):
            f = loss.vgg(torch.cat([c.x[p0:p0 + pp], c.y[p0:p0 + pp]]).cuda())
            fx.append(f[:f.shape[0] // 2])
            fy.append(f[f.shape[0] // 2:])
        own = F.mse_loss(torch.cat(fx).double(), torch.cat(fy).double()).item()
        print(f"  sqdiff: loss {got.item():.8e} vs fp64 mse of the returned features {own:.8e}")
        assert abs(got.item() - own) <= 1e-5 * own


def test_sqdiff_mean_kernel():
    """ragged sizes: n below one chunk, n across chunk boundaries, many pairs"""
    from mvd_amd import ops
    g = torch.Generator().manual_seed(3)
    for pairs, n in ((1, 4), (3, 4096 * 2 + 12), (5, 2 * 2 * 512), (2, 4096 * 300 + 4)):
        a, b = torch.randn(pairs, n, generator=g), torch.randn(pairs, n, generator=g)
        mean, pp = ops.sqdiff_mean(a.cuda(), b.cuda(), per_pair=True)
        want = ((a.double() - b.double()) ** 2).mean(1)
        assert (pp.double().cpu() - want).abs().max().item() <= 1e-6 * want.max().item(), (pairs, n)
        assert abs(mean.item() - want.mean().item()) <= 1e-6 * want.mean().item(), (pairs, n)
        again, _ = ops.sqdiff_mean(a.cuda(), b.cuda())
        assert torch.equal(again, mean)
    z, _ = ops.sqdiff_mean(a.cuda(), a.cuda())
    assert z.item() == 0.0


@pytest.mark.parametrize("pairs,h,w", R.SHAPES)
def test_identical_inputs_and_determinism(pairs, h, w):
    c = R.case(pairs, h, w)
    loss = make_loss(pairs)
    x, y = c.x.cuda(), c.y.cuda()
    zero = loss(x, x.clone())
    assert zero.item() == 0.0
    assert torch.equal(loss.per_sample(x, x.clone()), torch.zeros(pairs, device="cuda"))
    a, b = loss(x, y), loss(x, y)
    assert torch.equal(a, b) and a.item() > 0.0
    assert torch.equal(loss.per_sample(x, y), loss.per_sample(x, y))


@pytest.mark.parametrize("pairs,h,w", [s for s in R.SHAPES if s[0] > 1])
def test_per_sample(pairs, h, w):
    c = R.case(pairs, h, w)
    loss = make_loss(pairs)
    x, y = c.x.cuda(), c.y.cuda()
    per = loss.per_sample(x, y)
    assert per.shape == (pairs,) and per.is_cuda
    batch = loss(x, y).item()
    assert abs(per.double().mean().item() - batch) <= 1e-6 * batch
    for b in range(pairs):
        single = loss(x[b:b + 1], y[b:b + 1]).item()
        L, bound = loss_bound(2 * c.emu["conv5_3"], c.feat[b:b + 1], c.feat[pairs + b:pairs + b + 1])
        print(f"{(pairs, h, w)} pair {b}: per_sample {per[b].item():.6e}, single call {single:.6e}, fp32 tower {L:.6e}, bound {bound:.3e}")
        assert abs(per[b].item() - single) <= bound and abs(per[b].item() - L) <= bound


def test_errors_on_the_device(loss_fn):
    from mvd_amd._lib import MvdError
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    with pytest.raises(MvdError, match="must match"):
        loss_fn(x, torch.zeros(1, 3, 32, 48, device="cuda"))
    with pytest.raises(MvdError, match="16 x 16"):
        loss_fn(x[:, :, :8], x[:, :, :8])
    assert loss_fn(x.double(), x.double()).item() == 0.0                # other dtypes are converted, as .float() in compute_losses


def test_scorer_fills_perceptual_loss(loss_fn):
    """ValidationScorer(..., perceptual_loss_fn=PerceptualLoss(...)) on the tiny pipeline: the key is filled with what the loss
    gives on the decoded images"""
    from types import SimpleNamespace

    from mvd_amd import validation as V
    from mvd_amd.pipeline import MVDPipeline, _make_scheduler
    from tests import losses_ref as LR
    from tests.parity_util import build_pair, make_inputs

    class StandinVAE:
        config = SimpleNamespace(scaling_factor=LR.STANDIN_SCALING_FACTOR)

        def decode(self, z):
            return SimpleNamespace(sample=LR.standin_decode(z))

    ocfg, params, model = build_pair("tiny", 0, 96, 48)
    inp = make_inputs(ocfg, 2, 16, 7, 0, 96)                             # 16 x 16 latents -> 32 x 32 stand-in images
    model.fourier_projection = inp["proj"]
    pipe = MVDPipeline(model, _make_scheduler(None, "ddpm"))
    pipe.vae = StandinVAE()
    seen = {}

    def recording(x, y):
        seen["x"], seen["y"], seen["out"] = x, y, loss_fn(x, y)
        return seen["out"]

    scorer = V.ValidationScorer(pipe, perceptual_loss_fn=recording)
    assert scorer.vae is pipe.vae
    batch = dict(source_latents=inp["lat"], target_latents=inp["sample"] * 0.7, prompt_embeds=inp["text"], source_camera=inp["src"],
                 target_camera=inp["tgt"])
    noise = torch.randn(batch["target_latents"].shape, generator=torch.Generator().manual_seed(5))
    got = scorer.score(batch, noise=noise, timesteps=torch.tensor([7, 480]))
    v = got["perceptual_loss"]
    assert v.dim() == 0 and v.is_cuda and v.item() > 0.0 and torch.equal(v, seen["out"])
    assert tuple(seen["x"].shape) == (2, 3, 32, 32) and seen["x"].is_cuda
    # the decoded images are what the loss saw: the class itself, handed over directly, gives the same value
    assert torch.equal(loss_fn(seen["x"], seen["y"]), v)
    direct = V.ValidationScorer(pipe, perceptual_loss_fn=loss_fn).score(batch, noise=noise, timesteps=torch.tensor([7, 480]))["perceptual_loss"]
    # and the fp32 tower agrees within the loss bound
    fx, fy = R.features(R.synthetic_state_dict(), seen["x"].cpu()), R.features(R.synthetic_state_dict(), seen["y"].cpu())
    fe = R.features(R.synthetic_state_dict(), torch.cat([seen["x"], seen["y"]]).cpu(), emulate_bf16=True)
    L, bound = loss_bound(2 * R.rel_l2(fe, torch.cat([fx, fy])), fx, fy)
    print(f"scorer perceptual_loss {v.item():.6e}, fp32 tower {L:.6e}, bound {bound:.3e}")
    assert abs(v.item() - L) <= bound and abs(direct.item() - L) <= bound
    assert V.ValidationScorer(pipe).score(batch, noise=noise, timesteps=torch.tensor([7, 480]))["perceptual_loss"].item() == 0.0
