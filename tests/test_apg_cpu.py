"""Adaptive projected guidance (N19) without a GPU: the C ABI, the Python entry points, the ``APG`` value type, the plumbing of
``mvd_amd/val.py`` (stub pipeline, in the manner of test_guidance_rescale_cpu.py) and the identities that pin the fp64 restatement
of tests/apg_ref.py."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import n13_tree as T
from mvd_amd import _lib as L
from mvd_amd import val as V
from mvd_amd.scheduler import APG
from tests import apg_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvd_op_apg", "mvd_op_sampler_step_apg", "mvd_debug_apg_plan")


# ------------------------------------------------------------------------------------------------ C1
def test_header_declares_and_library_exports_the_apg_entry_points():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    declared = set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/mvd_hip.h"
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), f"{name} is not exported"
    # the argument checks run on the host, before any launch
    assert lib.mvd_op_apg(None, 3.0, 0.0, 0.0, 0.0, 0.0, None, None, 1, 256, None) == -1 and "apg" in L.last_error()
    assert lib.mvd_op_sampler_step_apg(None, 3.0, 0.0, 0.0, 0.0, 0.0, 0, None, None, None, None, 1, 0, 1, 0, 0, 0, None, None, 1, 256,
                                       None) == -1
    assert "sampler_step_apg" in L.last_error()


def test_host_checks_name_the_argument_before_any_launch():
    """made-up, never dereferenced addresses: every call here is refused by a host check"""
    lib = L.lib()
    mo, x, out, mom = (C.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20))

    def step(eta=0.0, tau=0.0, beta=0.0, phi=0.0, space=0, mom=None, out=out, x0_out=None, n_row=256, r=0.0, sigma=0.0):
        return lib.mvd_op_sampler_step_apg(mo, 3.0, eta, tau, beta, phi, space, mom, x, None, None, 1.0, 0.0, 1.0, 0.0, r, sigma, out,
                                           x0_out, 1, n_row, None)
    for kw, msg in ((dict(n_row=6), "multiple of 4"), (dict(eta=-0.1), "eta must lie in [0, 1]"), (dict(eta=1.5), "eta must lie"),
                    (dict(eta=float("nan")), "eta must lie"), (dict(tau=-1.0), "norm_threshold must be finite and >= 0"),
                    (dict(tau=float("nan")), "norm_threshold"), (dict(tau=float("inf")), "norm_threshold"),
                    (dict(beta=1.0), "momentum must lie in (-1, 1)"), (dict(beta=-1.0), "momentum must lie"),
                    (dict(beta=float("nan")), "momentum must lie"), (dict(phi=1.1), "guidance_rescale must lie in [0, 1]"),
                    (dict(phi=float("nan")), "guidance_rescale must lie"), (dict(beta=0.5), "momentum buffer required"),
                    (dict(space=1, phi=0.5), 'space="x0" with guidance_rescale > 0'), (dict(space=2), "space must be"),
                    (dict(r=0.5), "x0_prev required"), (dict(sigma=0.5), "noise required"),
                    (dict(out=mo), "overlaps the model output"), (dict(x0_out=C.c_void_p((1 << 20) + 1024)), "overlaps the model output"),
                    (dict(beta=0.5, mom=C.c_void_p((1 << 20) + 2047)), "overlaps the model output"),
                    (dict(beta=0.5, mom=x), "momentum buffer overlaps another argument"),
                    (dict(beta=0.5, mom=out), "momentum buffer overlaps another argument")):
        assert step(**kw) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    assert lib.mvd_op_apg(mo, 3.0, 0.0, 0.0, -0.5, 0.0, None, out, 1, 256, None) == -1 and "momentum buffer required" in L.last_error()
    assert lib.mvd_op_apg(mo, 3.0, 2.0, 0.0, 0.0, 0.0, None, out, 1, 256, None) == -1 and "apg: eta" in L.last_error()
    assert lib.mvd_op_apg(mo, 3.0, 0.0, 0.0, 0.5, 0.0, mom, mom, 1, 256, None) == -1 and "overlaps another argument" in L.last_error()


def test_plan_keeps_the_rows_the_rescale_kernel_keeps():
    from mvd_amd import ops
    for n in (256, 400, 960, 16384, 16388, 36864, 36868, 4 * 97 * 99, 40960):
        plan = ops.apg_plan(n)
        assert plan == ops.cfg_rescale_plan(n), n                  # the same KEEP rule, the same partition
        assert plan["threads"] == 1024 and plan["vec"] == 4 and plan["wave"] == 64
        assert plan["keep"] == (4 if n <= 16384 else 9 if n <= 36864 else 0)
    with pytest.raises(L.MvdError, match="multiple of 4"):
        ops.apg_plan(6)


# ------------------------------------------------------------------------------------------------ C2
def test_entry_points_take_apg_defaulting_to_none():
    from mvd_amd import ops
    from mvd_amd.pipeline import MVDDenoiser, MVDPipeline
    from mvd_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    for fn in (MVDDenoiser.__call__, MVDPipeline.__call__, MVDPipeline.generate_views, MVDPipeline.generate_views_batch):
        par = inspect.signature(fn).parameters["apg"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__
    for cls in (DDIMScheduler, DPMSolverMultistepScheduler):
        sig = inspect.signature(cls.step_guided).parameters
        assert sig["apg"].default is None and sig["momentum_buffer"].default is None
        assert sig["guidance_rescale"].default == 0.0
    assert not hasattr(DDPMScheduler, "step_guided") and callable(DDPMScheduler.step_guided_apg)
    sig = inspect.signature(DDPMScheduler.step_guided_apg).parameters
    assert list(sig)[:6] == ["self", "uncond_cond", "guidance_scale", "apg", "timestep", "sample"]
    assert sig["momentum_buffer"].default is None and sig["guidance_rescale"].default == 0.0
    # the schedulers hold no APG state
    for cls in (DDIMScheduler, DPMSolverMultistepScheduler, DDPMScheduler):
        assert not [k for k in vars(cls()) if "apg" in k.lower() or "momentum" in k.lower()]
    sig = inspect.signature(ops.sampler_step_apg).parameters
    assert [sig[k].default for k in ("eta", "norm_threshold", "momentum", "guidance_rescale", "space", "momentum_buffer")] == \
        [0.0, 0.0, 0.0, 0.0, "output", None]
    sig = inspect.signature(ops.apg).parameters
    assert [sig[k].default for k in ("eta", "norm_threshold", "momentum", "guidance_rescale", "momentum_buffer")] == [0.0, 0.0, 0.0, 0.0, None]
    for bad in (dict(eta=2.0), (0.0, -1.0, 0.0), "0,0,1.5", dict(space="latent")):
        with pytest.raises(ValueError, match="apg"):
            MVDDenoiser(None, None)(torch.zeros(1, 1, 1), apg=bad)
    with pytest.raises(ValueError, match='space="x0" with guidance_rescale'):
        MVDDenoiser(None, None)(torch.zeros(1, 1, 1), apg=APG(space="x0"), guidance_rescale=0.5)


def test_apg_value_type_validates_itself():
    a = APG()
    assert (a.eta, a.norm_threshold, a.momentum, a.space) == (0.0, 0.0, 0.0, "output")
    b = APG(0.5, 2.5, -0.5, "x0")
    assert APG.of(b) is b and APG.of(None) is None
    assert APG.of(dict(eta=0.5, norm_threshold=2.5, momentum=-0.5, space="x0")) == b
    assert APG.of((0.5, 2.5, -0.5, "x0")) == b and APG.of([0.5, 2.5, -0.5, "x0"]) == b and APG.of("0.5, 2.5, -0.5, x0") == b
    assert APG.of((0.5, 2.5, -0.5)) == APG(0.5, 2.5, -0.5) and APG.of("0.5,2.5,-0.5").space == "output"
    assert b != APG(0.5, 2.5, -0.5) and hash(b) == hash(APG(0.5, 2.5, -0.5, "x0")) and "norm_threshold=2.5" in repr(b)
    assert b.kwargs() == dict(eta=0.5, norm_threshold=2.5, momentum=-0.5)
    with pytest.raises(AttributeError):
        b.eta = 0.1
    for bad in (dict(eta=-0.01), dict(eta=1.01), dict(eta=float("nan")), dict(norm_threshold=-1e-9), dict(norm_threshold=float("inf")),
                dict(norm_threshold=float("nan")), dict(momentum=1.0), dict(momentum=-1.0), dict(momentum=float("nan")),
                dict(space="X0"), dict(space=None), dict(eta="a")):
        with pytest.raises(ValueError, match="apg"):
            APG(**bad)
    for bad in (dict(etta=0.5), (0.1, 0.2, 0.3, "x0", 5), (), "0.1;0.2", 0.5, object()):
        with pytest.raises(ValueError, match="apg"):
            APG.of(bad)
    # the edges of the ranges are what the definition allows
    APG(0.0, 0.0, 0.0)
    APG(1.0, 1e30, 0.999)
    APG(1.0, 0.0, -0.999)


# ------------------------------------------------------------------------------------------------ C3
class StubPipeline:
    """records its calls; every image is a function of its row's source image and target camera"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _images(source_images, target_camera):
        level = torch.tanh(target_camera.reshape(target_camera.shape[0], -1).sum(1)).abs().view(-1, 1, 1, 1)
        return (0.5 * source_images.clamp(-1, 1).add(1).div(2) + 0.5 * level).clamp(0, 1)

    def __call__(self, prompt=None, source_camera=None, target_camera=None, source_images=None, **kw):
        self.calls.append(("call", list(prompt), kw))
        return {"images": self._images(source_images, target_camera)}

    def generate_views_batch(self, prompts=None, source_images=None, source_cameras=None, target_cameras=None, **kw):
        self.calls.append(("batch", list(prompts), kw))
        rows = torch.repeat_interleave(torch.arange(len(target_cameras)), torch.tensor([t.shape[0] for t in target_cameras]))
        return {"images": self._images(source_images[rows], torch.cat(target_cameras))}


class StubMetrics:
    extra_metrics = ()

    def __init__(self):
        self.psnr = self.ssim = self.lpips_metric = self.perceptual_loss = lambda g, t: (g - t).abs().mean() + 1.0

    def calculate_metrics(self, g, t, prompts):
        return dict(psnr=1.0, ssim=1.0, perceptual_loss=1.0, lpips=1.0, clip_score=float(len(prompts)))

    def compute_fid(self):
        return 1.0


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    return T.build_tree(tmp_path_factory.mktemp("val_apg") / "data")


def _run(tree, out, **cfg):
    from mvd_amd.dataset import ObjaverseDataset
    ds = ObjaverseDataset(data_root=str(tree), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(32, 32), max_views_per_object=4,
                          frontend="host")
    config = dict(batch_size=6, num_workers=0, num_inference_steps=2, guidance_scale=2.0, ref_scale=0.1,
                  use_camera_conditioning=True, use_image_conditioning=True, **cfg)
    pipe = StubPipeline()
    V.run_validation(pipe, ds, config, "cpu", out, metrics=StubMetrics())
    return pipe.calls


@pytest.mark.parametrize("group", [False, True])
def test_val_passes_the_config_key_to_the_pipeline(tree, tmp_path, group):
    want = APG(0.0, 15.0, -0.5)
    for k, value in enumerate(("0,15,-0.5", [0.0, 15.0, -0.5], dict(eta=0.0, norm_threshold=15.0, momentum=-0.5))):
        calls = _run(tree, tmp_path / f"on{k}", apg=value, group_sources=group)
        assert calls and all(c[0] == ("batch" if group else "call") for c in calls)
        assert all(c[2]["apg"] == want and "guidance_rescale" not in c[2] for c in calls)
    calls = _run(tree, tmp_path / "both", apg="0.5,0,0,output", guidance_rescale=0.7, group_sources=group)
    assert calls and all(c[2]["apg"] == APG(0.5) and c[2]["guidance_rescale"] == 0.7 for c in calls)
    # off (absent, None or empty): the calls carry the arguments they always did
    for k, cfg in enumerate(({}, dict(apg=None), dict(apg=""))):
        calls = _run(tree, tmp_path / f"off{k}", group_sources=group, **cfg)
        assert calls and all("apg" not in c[2] for c in calls)
    with pytest.raises(ValueError, match="apg"):
        _run(tree, tmp_path / "bad", apg="0.5,2.5", group_sources=group)


def test_val_flag_overrides_the_config(monkeypatch, tmp_path):
    """``--apg`` through ``main``: the flag lands in the config that ``run_validation`` hands to the pipeline"""
    import mvd_amd.dataset as D
    seen = {}
    monkeypatch.setattr(V, "load_config", lambda path: dict(image_size=[32, 32], max_views_per_object=4, apg="1,0,0"))
    monkeypatch.setattr(V, "setup_pipeline", lambda config, ckpt, device: "pipe")
    monkeypatch.setattr(D, "ObjaverseDataset", lambda **kw: "dataset")

    def fake_run(pipeline, dataset, config, device, output_dir, **kw):
        seen.update(config)
        return [], {}
    monkeypatch.setattr(V, "run_validation", fake_run)
    argv = ["--ckpt", "x.ckpt", "--dataset-path", "data", "--output-dir", str(tmp_path)]
    assert V.main(argv + ["--apg", "0,2.5,-0.5,x0"]) == 0
    assert V.parse_apg(seen["apg"]) == APG(0.0, 2.5, -0.5, "x0")
    seen.clear()
    assert V.main(argv) == 0 and seen["apg"] == "1,0,0"                         # without the flag: the config's value
    for bad in ("0,2.5", "2,0,0", "0,0,0,latent"):
        with pytest.raises(SystemExit):
            V.main(argv + ["--apg", bad])
    assert V.parse_apg(None) is None and V.parse_apg("") is None


# ------------------------------------------------------------------------------------------------ C4
def _both(rows, shape, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2 * rows,) + shape, generator=g, dtype=torch.float64) * 1.7 + shift


def _dot(a, b):
    return (a.flatten(1) * b.flatten(1)).sum(1)


def test_restatement_identities():
    both = _both(5, (4, 6, 10), 1, shift=0.8)
    u, c = both.chunk(2)
    gs = 5.5
    # eta = 1, no cap, no momentum: plain classifier-free guidance
    m, _ = A.guided(both, gs, eta=1.0)
    plain = c + (gs - 1.0) * (c - u)
    assert ((m - plain).abs().max() / plain.abs().max()) <= 1e-14
    assert ((plain - (u + gs * (c - u))).abs().max() / plain.abs().max()) <= 1e-14
    # eta = 0: what is added to c is orthogonal to c
    for tau, beta in ((0.0, 0.0), (2.5, 0.0), (0.0, -0.5), (15.0, 0.5)):
        M = _both(5, (4, 6, 10), 7)[:5]
        m, _ = A.guided(both, gs, eta=0.0, norm_threshold=tau, momentum=beta, M=M)
        rel = _dot(m - c, c).abs() / ((m - c).flatten(1).norm(dim=1) * c.flatten(1).norm(dim=1))
        assert rel.max() <= 1e-12, (tau, beta, rel.max())
    # the cap: |s d| <= tau, rows under the threshold are untouched
    d = c - u
    norms = d.flatten(1).norm(dim=1)
    tau = float(norms.sort().values[2])                                     # the middle row's norm: two rows under, two over
    capped = A.cap(d, tau)
    cn = capped.flatten(1).norm(dim=1)
    assert bool((cn <= tau * (1 + 1e-14)).all()) and int((norms > tau).sum()) == 2
    assert torch.equal(capped[norms <= tau], d[norms <= tau]) and bool(((cn[norms > tau] - tau).abs() <= 1e-12 * tau).all())
    assert torch.equal(A.cap(d, 0.0), d) and torch.equal(A.cap(torch.zeros_like(d), 1.0), torch.zeros_like(d))
    # parallel + orthogonal = d, and a zero c has no parallel part
    par, orth = A.project(d, c)
    assert (par + orth - d).abs().max() <= 1e-14 and _dot(orth, c).abs().max() <= 1e-10
    par0, orth0 = A.project(d, torch.zeros_like(c))
    assert par0.abs().max() == 0.0 and torch.equal(orth0, d)
    # the rescale is N17's
    from tests import guidance_ref as G
    m, _ = A.guided(both, gs, eta=0.3, norm_threshold=tau)
    assert torch.allclose(A.rescale(m, c, 0.7), G.rescale_noise_cfg(m, c, 0.7), rtol=1e-14, atol=0)
    full, _ = A.guided(both, gs, eta=0.3, norm_threshold=tau, guidance_rescale=1.0)
    assert ((full.flatten(1).std(1) - c.flatten(1).std(1)).abs() / c.flatten(1).std(1)).max() <= 1e-12


@pytest.mark.parametrize("shift", [0.2, 8.0])
def test_five_sum_algebra_gives_the_moments_of_m(shift):
    """sum m and sum m^2 from the five sums against the sums of the m that tests/apg_ref.py builds by normalising c"""
    both = _both(6, (4, 12, 20), 3, shift=shift)
    u, c = both.chunk(2)
    M = _both(6, (4, 12, 20), 5)[:6]
    for gs, eta, tau, beta in ((7.5, 0.0, 0.0, 0.0), (3.0, 0.5, 60.0, -0.5), (12.0, 1.0, 2.5, 0.5), (1.0, 0.0, 15.0, 0.0), (5.0, 0.25, 80.0, 0.0)):
        m, d = A.guided(both, gs, eta=eta, norm_threshold=tau, momentum=beta, M=M)
        Ac, Bc, sm, smm = A.five_sum_moments(c, d, gs, eta, tau)
        direct = Ac.view(-1, 1, 1, 1) * c + Bc.view(-1, 1, 1, 1) * d
        assert ((direct - m).abs().max() / m.abs().max()) <= 1e-12
        s1, s2 = m.flatten(1).sum(1), (m * m).flatten(1).sum(1)
        assert ((sm - s1).abs() / s2.sqrt()).max() <= 1e-12 and ((smm - s2).abs() / s2).max() <= 1e-12, (gs, eta, tau, beta)
        # and the std the rescale needs, from those moments
        n = m[0].numel()
        var = (smm - sm * sm / n) / (n - 1)
        assert ((var.sqrt() - m.flatten(1).std(1)).abs() / m.flatten(1).std(1)).max() <= 1e-10


def test_momentum_recursion_is_the_geometric_sum():
    g = torch.Generator().manual_seed(4)
    steps, beta = 6, -0.5
    outs = [torch.randn(4, 4, 5, 6, generator=g, dtype=torch.float64) for _ in range(steps)]
    M = torch.zeros(2, 4, 5, 6, dtype=torch.float64)
    for t in range(steps):
        _, M = A.guided(outs[t], 3.0, momentum=beta, M=M)
        want = sum(beta ** k * (outs[t - k][2:] - outs[t - k][:2]) for k in range(t + 1))
        assert (M - want).abs().max() <= 1e-13
    # momentum 0 neither reads nor needs M
    m0, _ = A.guided(outs[0], 3.0, momentum=0.0, M=None)
    m1, _ = A.guided(outs[0], 3.0, momentum=0.0, M=torch.full((2, 4, 5, 6), 9.0, dtype=torch.float64))
    assert torch.equal(m0, m1)


def test_x0_space_is_output_space_on_the_denoised_predictions():
    both = _both(3, (4, 6, 6), 11, shift=0.3)
    x = _both(3, (4, 6, 6), 12)[:3]
    a0, a1 = -0.6, 0.8
    x0, M1 = A.guided_x0(both, x, a0, a1, 4.0, eta=0.0, norm_threshold=3.0, momentum=0.5, M=torch.ones(3, 4, 6, 6, dtype=torch.float64))
    u, c = both.chunk(2)
    assert torch.allclose(M1, a0 * (c - u) + 0.5, rtol=0, atol=1e-14)         # the sample cancels in d
    out, x0s, M2 = A.step(both, x, 4.0, a0, a1, 0.5, 0.4, eta=0.0, norm_threshold=3.0, momentum=0.5,
                          M=torch.ones(3, 4, 6, 6, dtype=torch.float64), space="x0")
    assert torch.equal(x0s, x0) and torch.equal(M2, M1) and torch.allclose(out, 0.5 * x + 0.4 * x0, rtol=0, atol=1e-14)
    # eta = 1 without a cap: both spaces give plain guidance, so the same step
    o1, z1, _ = A.step(both, x, 4.0, a0, a1, 0.5, 0.4, eta=1.0, space="x0")
    o2, z2, _ = A.step(both, x, 4.0, a0, a1, 0.5, 0.4, eta=1.0, space="output")
    assert torch.allclose(o1, o2, rtol=0, atol=1e-13) and torch.allclose(z1, z2, rtol=0, atol=1e-13)
    # the model output a textbook sampler takes in its place gives that x0 back
    mo, _ = A.as_model_output(both, x, a0, a1, 4.0, eta=0.0, norm_threshold=3.0, space="x0")
    want, _ = A.guided_x0(both, x, a0, a1, 4.0, eta=0.0, norm_threshold=3.0)
    assert torch.allclose(a0 * mo + a1 * x, want, rtol=0, atol=1e-13)
