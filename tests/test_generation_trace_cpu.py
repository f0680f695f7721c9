"""The call trace of the generation paths without a GPU: what ``MVDPipeline.__call__``, ``generate_views`` and both forms of
``generate_views_batch`` hand to the UNet, the VAE and the step ops, for every sampler and guidance setting.

A stub UNet and a stub VAE record their calls; ``mvd_amd.ops.ddpm_step`` / ``cfg_combine`` / ``cfg_rescale`` / ``sampler_step`` /
``sampler_step_rescaled`` are replaced by fp64 restatements on the host (tests/guidance_ref.py) that log the op name, the shape of
every tensor argument, which optional tensors were None and every scalar.  The traces in tests/golden/generation_trace.json were
recorded by ``python tests/test_generation_trace_cpu.py --record`` BEFORE the four entry points were folded onto one generation
path, with no product code changed; the sequence, the names, the shapes, the None pattern and the layout keywords are compared
exactly, the scalars (host float64 coefficients, which the kernels consume as fp32, one step of which is 6e-8) to a relative 1e-12
(another libm moves them by about 2e-16).

The scalars are functions of the fp32 schedule that ``_make_scheduler`` builds with torch's CPU kernels (log / exp / cumprod of
ShiftSNRScheduler), so they are as reproducible as that schedule is: a host on which tests/golden/g4_shift_snr.npz is not met
(test_next_rows_cpu.py) does not meet these either.  Names, shapes, None pattern and layout keywords do not depend on the host.

Two cases beyond the matrix: ``call/ddim/vae1`` gives ``__call__`` ONE source image for its two prompts (the repeat of
pipeline.py:106-107), ``call/own/g3neg`` a scheduler of the caller's whose ``step_guided`` has no ``guidance_rescale`` keyword."""
import inspect
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import guidance_ref as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "generation_trace.json")
STEPS, TEXT, DIM = 3, 7, 32

ENTRIES = ("call", "views3", "objects2x2", "objects1x2", "list21", "list22")
SAMPLERS = ("ddpm", "ddim", "dpmsolver++")
GUIDANCE = {
    "g1": dict(guidance_scale=1.0, negative=False, guidance_rescale=0.0),
    "g3neg": dict(guidance_scale=3.0, negative=True, guidance_rescale=0.0),
    "g3": dict(guidance_scale=3.0, negative=False, guidance_rescale=0.0),
    "g3rescale": dict(guidance_scale=3.0, negative=True, guidance_rescale=0.7),
}
EXTRA = ["call/ddim/vae1", "call/own/g3neg"]
CASES = [f"{e}/{s}/{g}" for e in ENTRIES for s in SAMPLERS for g in GUIDANCE] + [f"{e}/ddim/vae" for e in ENTRIES] + EXTRA


# ------------------------------------------------------------------------------------------------ the recorders
def _describe(v):
    """what the file holds of one argument: a tensor's shape (a list of ints), a scalar as a float, None, or the value itself"""
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    if v is None or isinstance(v, (bool, str, int, float)):
        return v
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _describe(x) for k, x in v.items()}
    return float(v)


class StubUNet:
    """enough of MultiViewUNet for the loop: records every call, returns a fixed function of ``sample``"""
    use_camera_conditioning = use_image_conditioning = True
    img_ref_scale = 0.3

    class config:
        sample_size = 2

    def __init__(self, log):
        self.log = log

    def _exec_device(self):
        return torch.device("cpu")

    def reset_reference_cache(self):
        self.log.append({"op": "unet.reset_reference_cache"})

    def __call__(self, **kw):
        ev = {"op": "unet", "timestep": float(kw["timestep"])}        # the keywords passed, by name: ``views`` / ``objects`` by value
        for k in sorted(kw):
            if k != "timestep":
                ev[k] = _describe(kw[k])
        self.log.append(ev)
        x = kw["sample"].float()
        rows = torch.arange(x.shape[0], dtype=torch.float32).view(-1, 1, 1, 1)
        return SimpleNamespace(sample=0.5 * x + 0.25 * x.flip(-1) + 0.01 * rows)


class StubVAE:
    """the AutoencoderKL protocol, 8x down and up by pooling; records the row counts"""
    config = SimpleNamespace(scaling_factor=0.18215)

    def __init__(self, log):
        self.log = log

    def encode(self, x):
        self.log.append({"op": "vae.encode", "rows": int(x.shape[0]), "shape": list(x.shape), "min": float(x.min()), "max": float(x.max())})
        z = torch.nn.functional.avg_pool2d(x.float(), 8).mean(1, keepdim=True).repeat(1, 4, 1, 1)
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda: z))

    def decode(self, z):
        self.log.append({"op": "vae.decode", "rows": int(z.shape[0]), "shape": list(z.shape)})
        return SimpleNamespace(sample=torch.nn.functional.interpolate(z[:, :3].float(), scale_factor=8))


def _affine(m, sample, a0, a1, p, q, r, sigma, x0_prev, noise, x0_out):
    x0 = a0 * m + a1 * sample.double()
    out = p * sample.double() + q * x0
    if r != 0.0:
        out = out + r * x0_prev.double()
    if sigma != 0.0:
        out = out + sigma * noise.double()
    if x0_out is not None:
        x0_out.copy_(x0.float())
    return out.float()


def ddpm_step(model_out, sample, noise, c0, c1, c2, c3, sigma):
    return _affine(model_out.double(), sample, c0, c1, c3, c2, 0.0, sigma, None, noise, None)


def cfg_combine(uncond_cond, guidance_scale):
    return G.guided(uncond_cond, guidance_scale).float()


def cfg_rescale(uncond_cond, guidance_scale, guidance_rescale, out=None):
    return G.guided(uncond_cond, guidance_scale, guidance_rescale).float()


def sampler_step(model_out, sample, a0, a1, p, q, r=0.0, sigma=0.0, x0_prev=None, noise=None, guidance_scale=None, out=None,
                 x0_out=None):
    m = model_out.double() if guidance_scale is None else G.guided(model_out, guidance_scale)
    return _affine(m, sample, a0, a1, p, q, r, sigma, x0_prev, noise, x0_out)


def sampler_step_rescaled(model_out, sample, guidance_scale, guidance_rescale, a0, a1, p, q, r=0.0, sigma=0.0, x0_prev=None,
                          noise=None, out=None, x0_out=None):
    return _affine(G.guided(model_out, guidance_scale, guidance_rescale), sample, a0, a1, p, q, r, sigma, x0_prev, noise, x0_out)


OPS = (ddpm_step, cfg_combine, cfg_rescale, sampler_step, sampler_step_rescaled)


def _recorded(fn, log):
    sig = inspect.signature(fn)

    def op(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        ev = {"op": fn.__name__}
        ev.update({k: _describe(v) for k, v in bound.arguments.items()})
        log.append(ev)
        return fn(*args, **kw)
    return op


# ------------------------------------------------------------------------------------------------ the cases
def _cam(*lead):
    n = 1
    for d in lead:
        n *= d
    c = torch.eye(4).repeat(n, 1, 1) + 0.01 * torch.arange(n, dtype=torch.float32).view(n, 1, 1)
    return c.reshape(*lead, 4, 4)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _entry(pipe, entry):
    """(bound method, its camera keywords) of one entry form"""
    if entry == "call":
        return pipe.__call__, dict(source_camera=_cam(2), target_camera=_cam(2))
    if entry == "views3":
        return pipe.generate_views, dict(source_camera=_cam(1)[0], target_cameras=_cam(3))
    if entry == "objects2x2":
        return pipe.generate_views_batch, dict(source_cameras=_cam(2), target_cameras=_cam(2, 2))
    if entry == "objects1x2":
        return pipe.generate_views_batch, dict(source_cameras=_cam(1), target_cameras=_cam(1, 2))
    counts = (2, 1) if entry == "list21" else (2, 2)
    return pipe.generate_views_batch, dict(source_cameras=_cam(2), target_cameras=[_cam(v) for v in counts])


# entry -> (prompt rows, latent rows, source rows)
LAYOUT = {"call": (2, 2, 2), "views3": (1, 3, 1), "objects2x2": (2, 4, 2), "objects1x2": (1, 2, 1), "list21": (2, 3, 2),
          "list22": (2, 4, 2)}


def _own_scheduler():
    """the shifted DDIM schedule in a class of the caller's, whose ``step_guided`` predates ``guidance_rescale``"""
    from mvd_amd.pipeline import _make_scheduler
    from mvd_amd.scheduler import DDIMScheduler

    class OwnScheduler(DDIMScheduler):
        def step_guided(self, uncond_cond, guidance_scale, timestep, sample, noise=None, generator=None):
            return super().step_guided(uncond_cond, guidance_scale, timestep, sample, noise=noise, generator=generator)

    ddim = _make_scheduler(None, "ddim")
    return OwnScheduler.from_config(ddim.config, trained_betas=ddim.betas.numpy())


def run_case(case, monkeypatch):
    from mvd_amd import ops
    from mvd_amd.pipeline import MVDPipeline, _make_scheduler
    entry, sampler, guidance = case.split("/")
    log = []
    for fn in OPS:
        monkeypatch.setattr(ops, fn.__name__, _recorded(fn, log))
    with_vae = guidance in ("vae", "vae1")
    g = GUIDANCE["g3neg" if with_vae else guidance]
    scheduler = _own_scheduler() if sampler == "own" else _make_scheduler(None, sampler)
    pipe = MVDPipeline(StubUNet(log), scheduler, vae=StubVAE(log) if with_vae else None)
    prompts, rows, sources = LAYOUT[entry]
    if guidance == "vae1":
        sources = 1
    fn, kw = _entry(pipe, entry)
    kw.update(prompt_embeds=_rand(1, prompts, TEXT, DIM), latents=_rand(2, rows, 4, 2, 2), num_inference_steps=STEPS,
              guidance_scale=g["guidance_scale"], guidance_rescale=g["guidance_rescale"])
    if g["negative"]:
        kw["negative_prompt_embeds"] = _rand(3, prompts, TEXT, DIM)
    if sampler == "ddpm":
        kw["noise_per_step"] = [_rand(10 + i, rows, 4, 2, 2) for i in range(STEPS)]
    if with_vae:
        kw.update(source_images=torch.rand(sources, 3, 16, 16, generator=torch.Generator().manual_seed(4)), output_type="pt")
    else:
        kw.update(source_image_latents=_rand(5, sources, 4, 2, 2), output_type="latent")
    out = fn(**kw)
    assert isinstance(out, dict) and list(out) == ["images"]
    assert torch.isfinite(out["images"]).all()
    log.append({"op": "return", "images": _describe(out["images"])})
    return log


# ------------------------------------------------------------------------------------------------ the comparison
def _same(got, want, where):
    if isinstance(want, float):
        assert isinstance(got, float), (where, got, want)
        assert got == want or abs(got - want) <= 1e-12 * max(abs(got), abs(want)), (where, got, want)
    elif isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (where, got, want)
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (where, got, want)
        for i, (a, b) in enumerate(zip(got, want)):
            _same(a, b, f"{where}[{i}]")
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES) and len(CASES) == 72 + 6 + len(EXTRA)


@pytest.mark.parametrize("case", CASES)
def test_generation_trace(case, golden, monkeypatch):
    got = json.loads(json.dumps(run_case(case, monkeypatch)))        # tuples -> lists, as the file holds them
    want = golden[case]
    assert [e["op"] for e in got] == [e["op"] for e in want], case
    _same(got, want, case)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_generation_trace_cpu.py --record")
    mp = pytest.MonkeyPatch()
    try:
        traces = {case: run_case(case, mp) for case in CASES}
    finally:
        mp.undo()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(t, separators=(',', ':'))}" for c, t in traces.items()) + "\n}\n")
    print(f"{len(traces)} traces -> {GOLDEN}")
