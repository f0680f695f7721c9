"""Guidance rescale (N17) without a GPU: the C ABI, the Python entry points, the plumbing of ``mvd_amd/val.py`` (stub pipeline, in
the manner of test_val_ragged_cpu.py) and the identities that pin the fp64 restatement of tests/guidance_ref.py."""
import inspect
import os
import re

import pytest
import torch

import n13_tree as T
from mvd_amd import _lib as L
from mvd_amd import val as V
from tests import guidance_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvd_op_cfg_rescale", "mvd_op_sampler_step_rescaled")


# ------------------------------------------------------------------------------------------------ C1
def test_header_declares_and_library_exports_the_rescale_entry_points():
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
    assert lib.mvd_op_cfg_rescale(None, 3.0, 0.5, None, 1, 256, None) == -1 and "cfg_rescale" in L.last_error()
    assert lib.mvd_op_sampler_step_rescaled(None, 3.0, 0.5, None, None, None, 1, 0, 1, 0, 0, 0, None, None, 1, 256, None) == -1
    assert "sampler_step_rescaled" in L.last_error()


def test_partition_offsets_come_from_the_launchers_constants():
    from mvd_amd import ops
    for n in (256, 400, 960, 16384, 36864, 40960):
        plan = ops.cfg_rescale_plan(n)
        offs = ops.cfg_rescale_partition(n)
        wchunk, per_pass = plan["wave"] * plan["vec"], plan["threads"] * plan["vec"]
        assert offs == sorted(set(offs)) and all(0 < o < n and o % plan["vec"] == 0 for o in offs)
        assert set(range(wchunk, n, wchunk)) <= set(offs) and set(range(per_pass, n, per_pass)) <= set(offs)
        assert set(range(plan["vec"], min(n, wchunk), plan["vec"])) <= set(offs)
        assert plan["passes"] == -(-n // per_pass)
        assert (plan["keep"] == 0) == (plan["passes"] > 9), plan        # 36864 floats is the longest row kept on chip
    assert ops.cfg_rescale_plan(16384)["keep"] * 1024 * 4 == 16384 and ops.cfg_rescale_plan(36864)["keep"] * 1024 * 4 == 36864
    with pytest.raises(L.MvdError, match="multiple of 4"):
        ops.cfg_rescale_plan(6)


# ------------------------------------------------------------------------------------------------ C2
def test_entry_points_take_guidance_rescale_defaulting_to_zero():
    from mvd_amd.pipeline import MVDDenoiser, MVDPipeline
    from mvd_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    for fn in (MVDDenoiser.__call__, MVDPipeline.__call__, MVDPipeline.generate_views, MVDPipeline.generate_views_batch):
        par = inspect.signature(fn).parameters["guidance_rescale"]
        assert par.default == 0.0 and par.kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__
    for cls in (DDIMScheduler, DPMSolverMultistepScheduler):
        assert inspect.signature(cls.step_guided).parameters["guidance_rescale"].default == 0.0
    assert not hasattr(DDPMScheduler, "step_guided") and not hasattr(DDPMScheduler(), "step_guided")
    assert callable(DDPMScheduler.step_guided_rescaled)
    # the shims re-export the same class
    import sys
    sys.path.insert(0, os.path.join(ROOT, "integration"))
    try:
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        from src.models.pipeline import MVDPipeline as Shim
        assert Shim is MVDPipeline
    finally:
        sys.path.remove(os.path.join(ROOT, "integration"))
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            MVDDenoiser(None, None)(torch.zeros(1, 1, 1), guidance_rescale=bad)


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
        self.calls.append(("call", list(prompt), None, None, None, kw))
        return {"images": self._images(source_images, target_camera)}

    def generate_views_batch(self, prompts=None, source_images=None, source_cameras=None, target_cameras=None, **kw):
        self.calls.append(("batch", list(prompts), None, None, None, kw))
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
    return T.build_tree(tmp_path_factory.mktemp("val_rescale") / "data")


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
    calls = _run(tree, tmp_path / "on", guidance_rescale=0.7, group_sources=group)
    assert calls and all(c[0] == ("batch" if group else "call") for c in calls)
    assert all(c[5]["guidance_rescale"] == 0.7 for c in calls)
    # off (absent or 0.0): the calls carry the arguments they always did
    for cfg in ({}, dict(guidance_rescale=0.0)):
        calls = _run(tree, tmp_path / f"off{len(cfg)}", group_sources=group, **cfg)
        assert calls and all("guidance_rescale" not in c[5] for c in calls)


@pytest.mark.parametrize("group", [False, True])
def test_val_flag_overrides_the_config(monkeypatch, tmp_path, group):
    """``--guidance-rescale`` through ``main``: the flag lands in the config that ``run_validation`` hands to the pipeline"""
    import mvd_amd.dataset as D
    seen = {}
    monkeypatch.setattr(V, "load_config", lambda path: dict(image_size=[32, 32], max_views_per_object=4, guidance_rescale=0.2))
    monkeypatch.setattr(V, "setup_pipeline", lambda config, ckpt, device: "pipe")
    monkeypatch.setattr(D, "ObjaverseDataset", lambda **kw: "dataset")

    def fake_run(pipeline, dataset, config, device, output_dir, **kw):
        seen.update(config)
        return [], {}
    monkeypatch.setattr(V, "run_validation", fake_run)
    argv = ["--ckpt", "x.ckpt", "--dataset-path", "data", "--output-dir", str(tmp_path)] + (["--group-sources"] if group else [])
    assert V.main(argv + ["--guidance-rescale", "0.6"]) == 0
    assert seen["guidance_rescale"] == 0.6 and bool(seen.get("group_sources")) == group
    seen.clear()
    assert V.main(argv) == 0 and seen["guidance_rescale"] == 0.2                # without the flag: the config's value


# ------------------------------------------------------------------------------------------------ C4
def _both(rows, shape, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2 * rows,) + shape, generator=g, dtype=torch.float64) * 1.7 + shift


def test_restatement_identities():
    both = _both(5, (4, 6, 10), 1, shift=0.8)
    u, c = both.chunk(2)
    gs = 5.5
    plain = u + gs * (c - u)
    # phi = 0 is the plain combine
    assert torch.equal(G.guided(both, gs, 0.0), plain)
    assert (G.rescale_noise_cfg(plain, c, 0.0) - plain).abs().max() == 0.0
    # phi = 1 makes every row's std the cond row's
    full = G.guided(both, gs, 1.0)
    s_full, s_c = full.flatten(1).std(1), c.flatten(1).std(1)
    assert ((s_full - s_c).abs() / s_c).max() <= 1e-12
    assert (plain.flatten(1).std(1) / s_c).min() > 1.5              # (the rescale had something to do)
    # in between: the blend of the two, so the std is the blend of the stds (the two are proportional)
    mid = G.guided(both, gs, 0.3)
    want = 0.3 * s_c + 0.7 * plain.flatten(1).std(1)
    assert ((mid.flatten(1).std(1) - want).abs() / want).max() <= 1e-12
    # unbiased std, written out
    x = c[0].flatten()
    assert abs(float(x.std()) - float(((x - x.mean()) ** 2).sum().div(x.numel() - 1).sqrt())) <= 1e-14
    # rows are independent: a row alone, or among other rows in another place, gives the same values (to the last bits of fp64:
    # torch may sum a row of another batch shape in another order)
    same = lambda a, b: bool(((a - b).abs() <= 1e-13 * b.abs()).all())      # noqa: E731
    for r in range(5):
        alone = G.guided(torch.cat([u[r:r + 1], c[r:r + 1]]), gs, 0.7)
        assert same(alone[0], G.guided(both, gs, 0.7)[r])
    perm = torch.tensor([3, 0, 4, 1, 2])
    assert same(G.guided(torch.cat([u[perm], c[perm]]), gs, 0.7), G.guided(both, gs, 0.7)[perm])
    changed = both.clone()
    changed[[1, 6]] += 3.0                                                  # another row 1: the other rows do not move
    keep = [0, 2, 3, 4]
    assert same(G.guided(changed, gs, 0.7)[keep], G.guided(both, gs, 0.7)[keep])
    # the fused step's restatement is the rescale followed by the affine step
    x, d, z = (torch.randn(5, 4, 6, 10, generator=torch.Generator().manual_seed(9 + i), dtype=torch.float64) for i in range(3))
    out, x0 = G.rescaled_step(both, gs, 0.7, x, -0.6, 0.8, 0.5, 0.4, r=-0.1, sigma=0.2, x0_prev=d, noise=z)
    m = G.guided(both, gs, 0.7)
    assert torch.equal(x0, -0.6 * m + 0.8 * x) and torch.allclose(out, 0.5 * x + 0.4 * x0 - 0.1 * d + 0.2 * z, rtol=0, atol=1e-14)


def test_restatement_has_no_epsilon():
    """a constant guided row has std 0: the quotient is what IEEE arithmetic gives (inf, or NaN for 0 / 0), as in diffusers"""
    c = torch.randn(1, 4, 4, 4, dtype=torch.float64)
    m = torch.full_like(c, 2.0)
    assert torch.isinf(G.rescale_noise_cfg(m, c, 0.5)).all()
    assert torch.isnan(G.rescale_noise_cfg(torch.zeros_like(c), c, 0.5)).all()
