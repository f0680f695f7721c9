"""DDIM / DPM-Solver++ on the MI355X: the fused step kernel (``mvd_op_sampler_step``), the schedulers' guided step, and the
loop through the pipeline against the CPU oracle (``oracle.mvd`` forward + ``tests/sampler_ref.py`` fp64 sampler).

Tolerances: the kernel against an fp64 restatement, relative <= 1e-6 (fp32 elementwise); the guided step against
cfg_combine + step, <= 1e-6; a 6-step tiny loop of chained bf16 UNet evaluations rel-L2 <= 4e-2 (as the DDPM loop of
tests/test_pipeline_gpu.py); the full-size loop as in the docstring of its test.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_util import build_pair
    return build_pair("tiny", 0, 96, 48)


@pytest.fixture()
def shim_path():
    p = os.path.join(ROOT, "integration")
    sys.path.insert(0, p)
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    yield p
    sys.path.remove(p)
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]


def _rel(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("n", [4, 4 * 13 * 17, 32 * 4 * 64 * 64])
@pytest.mark.parametrize("guided", [False, True])
def test_sampler_step_kernel(n, guided):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops
    g = torch.Generator().manual_seed(n + guided)
    mo = torch.randn((2 if guided else 1) * n, generator=g)
    x, d, z = (torch.randn(n, generator=g) for _ in range(3))
    for hist in (False, True):
        for noisy in (False, True):
            for alias in ("none", "out=sample", "x0_out=x0_prev"):
                if alias == "x0_out=x0_prev" and not hist:
                    continue
                a0, a1, p, q, r, sigma = (torch.rand(6, generator=g) * 4 - 2).tolist()
                r, sigma = (r if hist else 0.0), (sigma if noisy else 0.0)
                gs = 1.0 + 6.5 * torch.rand(1, generator=g).item()
                m = mo.double()
                if guided:
                    u, c = m.chunk(2)
                    m = u + gs * (c - u)
                x0 = a0 * m + a1 * x.double()
                want = p * x.double() + q * x0 + r * d.double() + sigma * z.double()
                xc, dc = x.cuda(), d.cuda()
                out = xc if alias == "out=sample" else None
                x0_out = dc if alias == "x0_out=x0_prev" else torch.empty(n, device="cuda")
                got = ops.sampler_step(mo.cuda(), xc, a0, a1, p, q, r, sigma, x0_prev=dc if hist else None,
                                       noise=z.cuda() if noisy else None, guidance_scale=gs if guided else None, out=out,
                                       x0_out=x0_out)
                torch.cuda.synchronize()
                if alias == "out=sample":
                    assert got.data_ptr() == xc.data_ptr()
                assert _rel(got, want) <= 1e-6, (hist, noisy, alias, _rel(got, want))
                assert _rel(x0_out, x0) <= 1e-6, (hist, noisy, alias)
    # errors come back through mvd_last_error, as mvd_op_ddpm_step's
    from mvd_amd._lib import MvdError
    with pytest.raises(MvdError, match="multiple of 4"):
        ops.sampler_step(torch.zeros(6, device="cuda"), torch.zeros(6, device="cuda"), 1, 0, 1, 0)
    with pytest.raises(MvdError, match="noise required"):
        ops.sampler_step(torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), 1, 0, 1, 0, sigma=0.5)
    with pytest.raises(MvdError, match="x0_prev required"):
        ops.sampler_step(torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), 1, 0, 1, 0, r=0.5)


def test_step_guided_equals_cfg_combine_then_step():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops
    from mvd_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, ShiftSNRScheduler
    g = torch.Generator().manual_seed(7)
    shape = (2, 4, 32, 32)
    for cls, kw in ((DDIMScheduler, dict(eta=0.0)), (DDIMScheduler, dict(eta=0.7)), (DPMSolverMultistepScheduler, {})):
        a = ShiftSNRScheduler.from_scheduler(DDPMScheduler(), "interpolated", shift_scale=6.0, scheduler_class=cls)
        b = ShiftSNRScheduler.from_scheduler(DDPMScheduler(), "interpolated", shift_scale=6.0, scheduler_class=cls)
        a.set_timesteps(8)
        b.set_timesteps(8)
        xa = xb = torch.randn(shape, generator=g).cuda()
        for t in a.timesteps.tolist():
            both = torch.randn((2 * shape[0],) + shape[1:], generator=g).cuda()
            nz = torch.randn(shape, generator=g).cuda()
            xa = a.step_guided(both, 5.0, t, xa, noise=nz, **kw).prev_sample
            xb = b.step(ops.cfg_combine(both, 5.0), t, xb, noise=nz, **kw).prev_sample
            torch.cuda.synchronize()
            assert _rel(xa, xb.double().cpu()) <= 1e-6, (cls.__name__, kw, t)


def _tiny_pipe(params, sampler=None):
    from src.models.mvd_unet import create_mvd_pipeline
    from mvd_amd.config import UNetConfig
    kw = {} if sampler is None else dict(sampler=sampler)
    pipe = create_mvd_pipeline(None, dtype=torch.float32, img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96,
                               cam_hidden_dim=48, unet_config=UNetConfig.tiny(), init="empty", **kw)
    missing, unexpected = pipe.unet.load_state_dict(params, strict=False)
    assert not missing and not unexpected
    pipe = pipe.to("cuda")
    pipe.unet.eval()
    return pipe


def _tiny_inputs(cfg, steps):
    from src.utils import create_camera_matrix
    from tests.parity_util import make_inputs
    B = 2
    inp = make_inputs(cfg, B, 16, 7, seed=31, cam_dim=96)
    src = create_camera_matrix([0, 0, 2.0], [0, 0, 0]).unsqueeze(0)           # infer.py:97-103: one 3x4 pair
    tgt = create_camera_matrix([1.5, 0, 1.5], [0, 0, 0]).unsqueeze(0)
    g = torch.Generator().manual_seed(5)
    noises = [torch.randn(B, 4, 16, 16, generator=g) for _ in range(steps)]
    neg = torch.randn(B, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(B, 4, 16, 16, generator=g)
    return inp, src, tgt, noises, neg, lat0


def _run_pipe(pipe, inp, src, tgt, noises, neg, lat0, steps, gs):
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    out = pipe(prompt_embeds=inp["text"].cuda(), negative_prompt_embeds=neg.cuda(), num_inference_steps=steps,
               guidance_scale=gs, latents=lat0.cuda(), source_camera=src, target_camera=tgt,
               source_image_latents=inp["lat"].cuda(), output_type="latent", noise_per_step=[n.cuda() for n in noises])
    return out["images"]


@pytest.mark.parametrize("sampler", ["ddim", "dpmsolver++"])
def test_pipeline_through_shims_with_sampler(tiny, shim_path, sampler):
    """``create_mvd_pipeline(..., sampler=)`` through the drop-in shims, CFG 3.0 (the guided step: ONE launch per step), one camera
    pair, source latents, 6 steps, against the oracle forward + the fp64 sampler restatement on the same grid."""
    from mvd_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    from tests import sampler_ref as R
    from tests.parity_util import rel_l2
    cfg, params, _ = tiny
    pipe = _tiny_pipe(params, sampler)
    assert type(pipe.scheduler) is (DDIMScheduler if sampler == "ddim" else DPMSolverMultistepScheduler)
    steps, gs = 6, 3.0
    inp, src, tgt, noises, neg, lat0 = _tiny_inputs(cfg, steps)
    c = pipe.scheduler.config
    ts = R.timesteps("ddim" if sampler == "ddim" else "dpm", c.num_train_timesteps, steps, c.timestep_spacing, c.steps_offset)
    want = R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"], neg, lat0, src, tgt, inp["lat"], sampler, ts, gs,
                          [inp["proj"]] * steps, set_alpha_to_one=getattr(c, "set_alpha_to_one", True), img_ref_scale=0.3,
                          cam_modulation_strength=0.2)
    got = _run_pipe(pipe, inp, src, tgt, noises, neg, lat0, steps, gs)
    assert pipe.scheduler.timesteps.tolist() == ts.tolist()
    assert torch.isfinite(got).all() and got.shape == lat0.shape
    err = rel_l2(got, want)
    print(f"{sampler}: tiny 6-step CFG-3 loop rel-L2 {err:.2e}", flush=True)
    assert err <= 4e-2, err


def test_ddpm_sampler_switch_is_the_default(tiny, shim_path):
    """``sampler="ddpm"`` is today's pipeline: the same latents, bit for bit, as the default."""
    cfg, params, _ = tiny
    steps, gs = 4, 3.0
    args = _tiny_inputs(cfg, steps)
    a = _run_pipe(_tiny_pipe(params), *args, steps, gs)
    b = _run_pipe(_tiny_pipe(params, "ddpm"), *args, steps, gs)
    assert torch.equal(a, b)


def test_sd21_full_size_dpmsolver_2m_loop():
    """DPM-Solver++ 2M at full SD-2.1 size (synthetic weights): 20 steps, guidance 1.0, B = 1, camera + image conditioning, the
    reference encoder re-run every step, Q1's projection pinned, against the oracle forward + the fp64 sampler restatement,
    checked on the WHOLE trajectory.  Deterministic samplers lack DDPM's damping of the forward's error, so the bound is an
    estimate: final rel-L2 <= 3e-2, no step multiplies the accumulated error by more than 1.5 (+2e-3).  Measured on the MI355X,
    rel-L2 per step: 1.1e-4 2.2e-4 3.1e-4 4.3e-4 5.7e-4 7.3e-4 9.2e-4 1.1e-3 1.4e-3 1.6e-3 1.9e-3 2.2e-3 2.5e-3 2.8e-3 3.0e-3
    3.3e-3 3.4e-3 3.5e-3 3.7e-3 4.0e-3.  ~60 s of CPU oracle on 16 threads."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd.pipeline import MVDDenoiser
    from mvd_amd.scheduler import DDPMScheduler, DPMSolverMultistepScheduler, ShiftSNRScheduler
    from tests import sampler_ref as R
    from tests.parity_util import make_inputs, rel_l2, shared_pair
    cfg, params, model = shared_pair("sd21")
    inp = make_inputs(cfg, 1, 64, 77, seed=43, cam_dim=1024)
    sched = ShiftSNRScheduler.from_scheduler(DDPMScheduler(), "interpolated", shift_scale=6.0,
                                             scheduler_class=DPMSolverMultistepScheduler)
    steps, gs = 20, 1.0
    lat0 = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(8))
    ts = R.timesteps("dpm", 1000, steps, sched.config.timestep_spacing, sched.config.steps_offset)
    want_tr = []
    R.denoise_loop(params, cfg, sched.betas, inp["text"], None, lat0, inp["src"], inp["tgt"], inp["lat"], "dpmsolver++", ts, gs,
                   [inp["proj"]] * steps, trace=want_tr, img_ref_scale=0.3, cam_modulation_strength=0.2)
    model.fourier_projection = inp["proj"]
    got_tr = []
    try:
        den = MVDDenoiser(model, sched)
        den(inp["text"].cuda(), steps, gs, latents=lat0.cuda(), source_camera=inp["src"].cuda(), target_camera=inp["tgt"].cuda(),
            source_image_latents=inp["lat"].cuda(), callback=lambda i, t, l: got_tr.append(l.float().cpu().clone()))
    finally:
        model.fourier_projection = None
    assert sched.timesteps.tolist() == ts.tolist()
    assert len(got_tr) == steps == len(want_tr)
    errs = [rel_l2(a, b) for a, b in zip(got_tr, want_tr)]
    print("full-size DPM-Solver++ 2M 20-step guidance-1.0 loop, rel-L2 per step = " + " ".join(f"{e:.1e}" for e in errs),
          flush=True)
    assert all(torch.isfinite(t).all() for t in got_tr)
    assert errs[-1] <= 3e-2, errs[-5:]
    for i in range(1, steps):
        assert errs[i] <= 1.5 * errs[i - 1] + 2e-3, (i, errs[i - 1], errs[i])
