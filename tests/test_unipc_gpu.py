"""UniPC on the MI355X: the fused corrector + predictor kernel (``mvd_op_unipc_step``) against the fp64
restatement of its formula (tests/unipc_ref.py ``kernel_map``), the scheduler's guided step against cfg_combine + step, and the
loop through the pipeline against the CPU oracle (``oracle.mvd`` forward + the textbook fp64 UniPC of tests/unipc_ref.py).

The kernel's bound, per element: k * 2^-24 * A, A the sum of |coefficient * term| over the output's terms (every intermediate
replaced by its own A) from the restatement, k the number of fp32 operations on the output's longest path in the documented
evaluation order (include/mvd_hip.h): m = fma(c - u, g, u) is 2, x0 = fma(a0, m, a1*x) 2 more (K_X0 = 4), xc = cx*xl and four fma
5 more (K_XC = 9), y = px*xc and three fma 4 more (K_Y = 13).  Every operation rounds its result by at most 2^-24 relative, and
the result's magnitude is at most the A of its terms, so the bound holds to first order in 2^-24 whatever the inputs; the
coefficients are rounded to fp32 before both sides use them.  The 6-step tiny loop of chained bf16 UNet evaluations: rel-L2 <=
4e-2, test_pipeline_through_shims_with_sampler's bound."""
import os
import sys

import pytest
import torch

from tests import unipc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
K_X0, K_XC, K_Y = 4, 9, 13
NAMES = ("a0", "a1", "cx", "c0", "c1", "c2", "ct", "px", "p0", "p1", "p2")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _within(got, want, A, k, what):
    excess = ((got.double() - want).abs() - k * U24 * A).max().item()
    assert excess <= 0.0, (what, excess)


ALIASES = ("none", "y=x", "xc=xl", "x0=h0", "x0=h1", "x0=h2", "all")


@pytest.mark.parametrize("n", [4, 4 * 257, 4 * (256 * 2048 + 3)])      # one vector; a partial second block; past the grid cap
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("corr", [False, True])
def test_unipc_step_kernel(n, guided, corr):
    _gpu()
    from mvd_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + 2 * guided + corr)
    rnd = lambda m: torch.randn(m, generator=g, device="cuda")      # noqa: E731
    mo, x, xl = rnd((2 if guided else 1) * n), rnd(n), rnd(n)
    hs = [rnd(n) for _ in range(3)]
    mo64, x64, xl64, hs64 = mo.double(), x.double(), xl.double(), [t.double() for t in hs]
    for depth in (0, 1, 2, 3):                                      # how many x0 predictions the history holds
        for alias in ALIASES:
            if alias.startswith("x0=h") and int(alias[-1]) >= depth:
                continue
            k = dict(zip(NAMES, (torch.rand(len(NAMES), generator=g, device="cuda") * 4 - 2).tolist()))    # fp32 values in [-2, 2]
            for name, need in (("c0", 1), ("p1", 1), ("c1", 2), ("p2", 2), ("c2", 3)):
                if depth < need:
                    k[name] = 0.0
            if not corr:
                k.update(cx=0.0, c0=0.0, c1=0.0, c2=0.0, ct=0.0)
            gs = (1.0 + 6.5 * torch.rand(1, generator=g, device="cuda")).item() if guided else None         # an fp32 value
            used = [k["c0"] != 0.0 or k["p1"] != 0.0, k["c1"] != 0.0 or k["p2"] != 0.0, k["c2"] != 0.0]
            want = R.kernel_map(mo64, x64, xl64 if corr else None, [t if u else None for t, u in zip(hs64, used)], k, corr, gs)
            xa, xla, ha = x.clone(), xl.clone(), [t.clone() for t in hs]
            out = xa if alias in ("y=x", "all") else None
            xc_out = xla if alias in ("xc=xl", "all") else torch.empty(n, device="cuda")
            slot = depth - 1 if alias == "all" else int(alias[-1]) if alias.startswith("x0=h") else -1
            x0_out = ha[slot] if slot >= 0 else torch.empty(n, device="cuda")
            got = ops.unipc_step(mo, xa, k["a0"], k["a1"], k["px"], k["p0"], k["p1"], k["p2"], corr=corr, cx=k["cx"], c0=k["c0"],
                                 c1=k["c1"], c2=k["c2"], ct=k["ct"], last_sample=xla if corr else None,
                                 h0=ha[0] if depth >= 1 else None, h1=ha[1] if depth >= 2 else None,
                                 h2=ha[2] if depth >= 3 else None, guidance_scale=gs, out=out, xc_out=xc_out, x0_out=x0_out)
            torch.cuda.synchronize()
            if out is not None:
                assert got.data_ptr() == xa.data_ptr()
            what = (depth, alias)
            _within(got, want[0], want[3], K_Y, what + ("y",))
            _within(xc_out, want[1], want[4], K_XC, what + ("xc",))
            _within(x0_out, want[2], want[5], K_X0, what + ("x0",))
            if not corr:
                assert torch.equal(xc_out, x), what                # without the corrector xc IS the sample
            # nothing but the outputs is written
            assert torch.equal(mo.double(), mo64)
            for j, t in enumerate(ha):
                assert j == slot or torch.equal(t, hs[j]), what + (j,)
            assert alias in ("y=x", "all") or torch.equal(xa, x)
            assert alias in ("xc=xl", "all") or torch.equal(xla, xl)


def test_unipc_step_errors_come_back_through_mvd_last_error():
    _gpu()
    from mvd_amd import ops
    from mvd_amd._lib import MvdError
    z = lambda m=8: torch.zeros(m, device="cuda")       # noqa: E731
    with pytest.raises(MvdError, match="multiple of 4"):
        ops.unipc_step(z(6), z(6), 1, 0, 1, 0)
    with pytest.raises(MvdError, match="h0 required"):
        ops.unipc_step(z(), z(), 1, 0, 1, 0, p1=0.5)
    with pytest.raises(MvdError, match="h1 required"):
        ops.unipc_step(z(), z(), 1, 0, 1, 0, p2=0.5, h0=z())
    with pytest.raises(MvdError, match="h2 required"):
        ops.unipc_step(z(), z(), 1, 0, 1, 0, corr=True, cx=1.0, c2=0.5, last_sample=z())
    with pytest.raises(MvdError, match="last_sample required"):
        ops.unipc_step(z(), z(), 1, 0, 1, 0, corr=True, cx=1.0)
    mo = z(16)
    for kw in (dict(out=mo[8:]), dict(xc_out=mo[:8]), dict(x0_out=mo[4:12])):
        with pytest.raises(MvdError, match="overlaps the model output"):
            ops.unipc_step(mo, z(), 1, 0, 1, 0, guidance_scale=2.0, **kw)
    with pytest.raises(MvdError, match="overlaps the model output"):
        ops.unipc_step(mo[:8], z(), 1, 0, 1, 0, out=mo[:8])
    buf = z()
    with pytest.raises(MvdError, match="overlap one another"):
        ops.unipc_step(z(), z(), 1, 0, 1, 0, xc_out=buf, x0_out=buf)


def _shifted_unipc(**kw):
    from mvd_amd.scheduler import DDPMScheduler, ShiftSNRScheduler, UniPCMultistepScheduler
    from types import SimpleNamespace
    base = DDPMScheduler()
    base.config = SimpleNamespace(**{**vars(base.config), **kw})
    return ShiftSNRScheduler.from_scheduler(base, "interpolated", shift_scale=6.0, scheduler_class=UniPCMultistepScheduler)


@pytest.mark.parametrize("order", [2, 3])
def test_step_guided_equals_cfg_combine_then_step(order):
    """Along a 6-step grid, ``step_guided`` (ONE launch) and ``cfg_combine`` + ``step`` (two) from the same state: each lies within the
    kernel's bound of the fp64 restatement of the call (the two-launch path within K_Y + 1: cfg_combine's u + (c - u)*g may take
    three roundings where the fused fma(c - u, g, u) takes two), so they lie within the sum of the two of each other.  The
    second scheduler's state is copied from the first before every call, so that every call is held to the bound on its own."""
    _gpu()
    from mvd_amd import ops
    g = torch.Generator().manual_seed(7)
    shape, gs = (2, 4, 32, 32), 5.0
    key = (shape, torch.device("cuda", torch.cuda.current_device()))
    a, b = _shifted_unipc(solver_order=order), _shifted_unipc(solver_order=order)
    a.set_timesteps(6)
    b.set_timesteps(6)
    x = torch.randn(shape, generator=g).cuda()
    for i, t in enumerate(a.timesteps.tolist()):
        both = torch.randn((2 * shape[0],) + shape[1:], generator=g).cuda()
        c = a.step_coefficients(i)
        k = {name: float(torch.tensor(getattr(c, name), dtype=torch.float32)) for name in NAMES}
        if i > 0:
            key = next(iter(a._bufs))
            for dst, src in zip(b._bufs[key][0] + [b._bufs[key][1]], a._bufs[key][0] + [a._bufs[key][1]]):
                dst.copy_(src)
            hist, last = a._bufs[key]
            used = [k["c0"] != 0.0 or k["p1"] != 0.0, k["c1"] != 0.0 or k["p2"] != 0.0, k["c2"] != 0.0]
            h64 = [hist[j].double().flatten() if j < order and used[j] else None for j in range(3)]
            xl64 = last.double().flatten() if c.corr else None
        else:
            h64, xl64 = [None] * 3, None
        assert c.corr == (i > 0)
        want, _, _, A, _, _ = R.kernel_map(both.double().flatten(), x.double().flatten(), xl64, h64, k, c.corr,
                                           float(torch.tensor(gs, dtype=torch.float32)))
        ya = a.step_guided(both, gs, t, x).prev_sample
        yb = b.step(ops.cfg_combine(both, gs), t, x).prev_sample
        torch.cuda.synchronize()
        _within(ya.flatten(), want, A, K_Y, (i, "step_guided"))
        _within(yb.flatten(), want, A, K_Y + 1, (i, "cfg_combine + step"))
        _within(ya.flatten(), yb.double().flatten(), A, 2 * K_Y + 1, (i, "one against the other"))
        x = ya
    assert a.step_index == b.step_index == 6


# ------------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def tiny():
    _gpu()
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


def _tiny_pipe(params, sampler):
    from src.models.mvd_unet import create_mvd_pipeline
    from mvd_amd.config import UNetConfig
    pipe = create_mvd_pipeline(None, dtype=torch.float32, img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96,
                               cam_hidden_dim=48, unet_config=UNetConfig.tiny(), init="empty", sampler=sampler)
    missing, unexpected = pipe.unet.load_state_dict(params, strict=False)
    assert not missing and not unexpected
    pipe = pipe.to("cuda")
    pipe.unet.eval()
    return pipe


def _run_pipe(pipe, inp, src, tgt, neg, lat0, steps, gs):
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    return pipe(prompt_embeds=inp["text"].cuda(), negative_prompt_embeds=neg.cuda(), num_inference_steps=steps, guidance_scale=gs,
                latents=lat0.cuda(), source_camera=src, target_camera=tgt, source_image_latents=inp["lat"].cuda(),
                output_type="latent")["images"]


PIPE_TOL = 4e-2


def test_pipeline_through_shims_with_unipc(tiny, shim_path):
    """``create_mvd_pipeline(..., sampler="unipc")`` through the drop-in shims, CFG 3.0 (corrector, predictor and the guidance
    combine: ONE launch per step), one camera pair, source latents, 6 steps, against the oracle forward + the textbook fp64 UniPC
    on the same grid: rel-L2 <= 4e-2.  Only if UniPC misses that bound is the ``dpmsolver++`` arm measured in the same run and
    1.5 x its value allowed (the corrector uses each bf16 model output in two updates).  The oracle's own DPM-Solver++ 2M result
    on this grid lies 5.8e-2 from its UniPC result (CPU, fp64 samplers): the pipeline's result has to lie nearer the UniPC one, so
    that a loop which ran no corrector could not pass unnoticed.
    Measured on the MI355X: rel-L2 2.05e-2 to the oracle's UniPC result (the fallback arm did not run)."""
    from mvd_amd import _lib as L
    from mvd_amd.scheduler import UniPCMultistepScheduler
    from src.utils import create_camera_matrix
    from tests import sampler_ref as S
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, _ = tiny
    pipe = _tiny_pipe(params, "unipc")
    assert type(pipe.scheduler) is UniPCMultistepScheduler
    steps, gs, B = 6, 3.0, 2
    inp = make_inputs(cfg, B, 16, 7, seed=31, cam_dim=96)
    src = create_camera_matrix([0, 0, 2.0], [0, 0, 0]).unsqueeze(0)           # infer.py:97-103: one 3x4 pair
    tgt = create_camera_matrix([1.5, 0, 1.5], [0, 0, 0]).unsqueeze(0)
    g = torch.Generator().manual_seed(5)
    neg = torch.randn(B, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(B, 4, 16, 16, generator=g)
    c = pipe.scheduler.config
    ts = R.timesteps("dpm", c.num_train_timesteps, steps, c.timestep_spacing, c.steps_offset)
    oracle_kw = dict(img_ref_scale=0.3, cam_modulation_strength=0.2)
    want = R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"], neg, lat0, src, tgt, inp["lat"], ts, gs, [inp["proj"]] * steps,
                          **oracle_kw)
    want_2m = S.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"], neg, lat0, src, tgt, inp["lat"], "dpmsolver++", ts, gs,
                             [inp["proj"]] * steps, **oracle_kw)
    moved = rel_l2(want_2m, want)
    launches = []
    real_call = L.call
    L.call = lambda name, *a: (launches.append(name), real_call(name, *a))[1]
    try:
        got = _run_pipe(pipe, inp, src, tgt, neg, lat0, steps, gs)
    finally:
        L.call = real_call
    assert pipe.scheduler.timesteps.tolist() == ts.tolist()
    assert torch.isfinite(got).all() and got.shape == lat0.shape
    assert launches.count("mvd_op_unipc_step") == steps
    assert not [n for n in launches if n in ("mvd_op_cfg_combine", "mvd_op_sampler_step", "mvd_op_ddpm_step")]
    err = rel_l2(got, want)
    print(f"unipc: tiny 6-step CFG-3 loop rel-L2 {err:.2e}; the oracle's DPM-Solver++ 2M result is {moved:.2e} away", flush=True)
    bound = PIPE_TOL
    if err > bound:
        dpm = _tiny_pipe(params, "dpmsolver++")
        err_2m = rel_l2(_run_pipe(dpm, inp, src, tgt, neg, lat0, steps, gs), want_2m)
        print(f"dpmsolver++: the same loop rel-L2 {err_2m:.2e}", flush=True)
        bound = 1.5 * err_2m
    assert err <= bound, (err, bound)
    assert err < rel_l2(got, want_2m), (err, rel_l2(got, want_2m))
