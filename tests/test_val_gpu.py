"""``mvd_amd.val.run_validation`` end to end on the MI355X: the synthetic Objaverse tree of tests/n13_tree.py, the tiny snapshot of
tests/text_fixture.py (UNet, VAE, native text encoder), seeded metric weights and the CLIP fixture; 2 batches of 2 pairs, 64 x 64
images, 2 steps.  Both CSV files exist with the reference's columns in order; every per-batch and per-sample value equals a direct
call of the metric class on the same tensors, bit for bit; with ``extra_metrics`` the shared-tower values equal separately fed
metrics.  Without mvd_amd/val.py this file fails at import."""
import csv

import pytest
import torch

import n13_tree as T
from mvd_amd import val as V

pytestmark = pytest.mark.gpu

COLUMNS = ["object_uid", "prompt", "inference_time_seconds", "psnr", "ssim", "perceptual_loss", "lpips", "clip_score",
           "batch_inference_time_seconds", "num_samples_in_batch"]
REFERENCE_ROWS = [f"{m}_{s}" for m in ("psnr", "ssim", "perceptual_loss", "lpips") for s in ("mean", "std", "min", "max")] + \
    ["fid", "clip_score_mean", "clip_score_std", "mean_batch_inference_time_seconds", "std_batch_inference_time_seconds",
     "min_batch_inference_time_seconds", "max_batch_inference_time_seconds", "total_inference_duration_seconds",
     "total_samples_processed_in_inference", "avg_per_sample_inference_time_seconds"]
EXTRA_ROWS = ["kid_mean", "kid_std", "inception_score_mean", "inception_score_std", "precision", "recall", "f_score", "density", "coverage"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pytest.importorskip("PIL")
    from tests import fid_ref, lpips_ref, vgg_ref
    from tests.clip_fixture import build_clip_snapshot
    from tests.hub_fixture import REPO
    from tests.text_fixture import build_text_snapshot
    tmp = tmp_path_factory.mktemp("val")
    cache, _, _, _ = build_text_snapshot(str(tmp / "hf"))
    clip_snap, _ = build_clip_snapshot(tmp / "clip")
    ckpt = tmp / "last.ckpt"
    torch.save({"state_dict": {}}, ckpt)          # (no unet.* keys: the snapshot's weights stay; the loader is what is exercised)
    config = dict(architecture=REPO, cache_dir=cache, torch_dtype="float32", use_camera_conditioning=True, use_image_conditioning=True,
                  img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96, cam_hidden_dim=48, simple_encoder=False,
                  image_size=[64, 64], max_views_per_object=2, batch_size=2, num_workers=0, num_inference_steps=2, guidance_scale=2.0,
                  ref_scale=0.1, clip_model_name=clip_snap, sampler="ddim")
    pipe = V.setup_pipeline(config, str(ckpt), "cuda")
    pipe.unet.config.sample_size = 32             # 32 x 32 latents under the fixture's 2x VAE: 64 x 64 images
    weights = dict(perceptual_weights=vgg_ref.synthetic_state_dict(), lpips_backbone=lpips_ref.backbone("alex"),
                   lpips_model_path=lpips_ref.synthetic_lins("alex"), inception_weights=fid_ref.synthetic_inception_state_dict(0))
    root = T.build_tree(tmp / "data")
    return config, pipe, weights, root


def dataset(root, frontend):
    from mvd_amd.dataset import ObjaverseDataset
    return ObjaverseDataset(data_root=str(root), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(64, 64), max_views_per_object=2,
                            dataset_samples=4, frontend=frontend)


def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def run(setup, out, frontend, **kw):
    config, pipe, weights, root = setup
    seen = []
    ds = dataset(root, frontend)
    assert len(ds) == 4
    torch.manual_seed(123)
    results, overall = V.run_validation(pipe, ds, config, "cuda", out, metric_kwargs=weights,
                                        on_batch=lambda i, g, t, p: seen.append((i, g.clone(), t.clone(), list(p))), **kw)
    return results, overall, seen


def test_run_validation_writes_the_references_files(setup, tmp_path):
    results, overall, seen = run(setup, tmp_path, "device")
    assert [i for i, *_ in seen] == [0, 1] and all(g.shape == (2, 3, 64, 64) and g.is_cuda for _, g, _, _ in seen)
    rows = read_csv(tmp_path / "validation_results.csv")
    assert rows[0] == COLUMNS and len(rows) == 1 + 4 and list(results[0].keys()) == COLUMNS
    orows = read_csv(tmp_path / "overall_metrics.csv")
    assert orows[0] == ["Metric", "Value"] and [r[0] for r in orows[1:]] == REFERENCE_ROWS == list(overall.keys())
    assert [r[1] for r in orows[1:]] == [str(v) for v in overall.values()]
    assert sorted(p.name for p in (tmp_path / "samples").iterdir()) == sorted(
        f"comparison_batch{b:04d}_uid_{results[2 * b + 1]['object_uid']}.png" for b in (0, 1))          # the last sample of each batch
    # every value against a direct call of the metric class on the same tensors
    _, _, weights, _ = setup
    direct = V.ValidationMetrics("cuda", setup[0]["clip_model_name"], **weights)
    per_batch = []
    for b, gen, tgt, prompts in seen:
        want = dict(psnr=direct.psnr(gen, tgt).item(), ssim=direct.ssim(gen, tgt).item(), perceptual_loss=direct.perceptual_loss(gen, tgt).item(),
                    lpips=direct.lpips_metric(gen, tgt).mean().item(),
                    clip_score=direct.clip_score_metric(((gen.clamp(-1, 1) + 1) / 2.0 * 255).to(torch.uint8), prompts).item())
        direct.fid_metric.update((gen.clamp(-1, 1) + 1) / 2.0, real=False)
        direct.fid_metric.update((tgt.clamp(-1, 1) + 1) / 2.0, real=True)
        per_batch.append(want)
        for i in range(2):
            r = results[2 * b + i]
            assert r["prompt"] == prompts[i] and r["clip_score"] == want["clip_score"] and r["num_samples_in_batch"] == 2
            assert r["inference_time_seconds"] == r["batch_inference_time_seconds"] / 2 > 0
            assert r["psnr"] == direct.psnr(gen[i:i + 1], tgt[i:i + 1]).item()
            assert r["ssim"] == direct.ssim(gen[i:i + 1], tgt[i:i + 1]).item()
            assert r["lpips"] == direct.lpips_metric(gen[i:i + 1], tgt[i:i + 1]).item()
            assert r["perceptual_loss"] == direct.perceptual_loss(gen[i:i + 1], tgt[i:i + 1]).item()
    times = [dict(batch_inference_time_seconds=results[2 * b]["batch_inference_time_seconds"], num_samples_in_batch=2) for b in (0, 1)]
    want_overall = V.calculate_overall_metrics([dict(m, **t) for m, t in zip(per_batch, times)], direct.fid_metric.compute().item())
    assert list(want_overall) == list(overall)
    for k in overall:
        assert float(overall[k]) == float(want_overall[k]), k
    assert all(m["psnr"] > 0 and 0 < m["lpips"] for m in per_batch) and overall["fid"] > 0


def test_host_and_device_front_ends_give_the_same_run(setup, tmp_path):
    a = run(setup, tmp_path / "host", "host")
    b = run(setup, tmp_path / "device", "device")
    for (_, ga, ta, pa), (_, gb, tb, pb) in zip(a[2], b[2]):
        assert torch.equal(ta, tb) and torch.equal(ga, gb) and pa == pb
    timing = ("inference_time_seconds", "batch_inference_time_seconds")
    for ra, rb in zip(a[0], b[0]):
        assert {k: v for k, v in ra.items() if k not in timing} == {k: v for k, v in rb.items() if k not in timing}


def test_extra_metrics_share_one_tower(setup, tmp_path):
    from mvd_amd.fid import FrechetInceptionDistance
    from mvd_amd.kid import InceptionScore, KernelInceptionDistance
    from mvd_amd.prdc import DensityCoverage, PrecisionRecall
    config, _, weights, _ = setup
    small = dict(kid_subsets=5, kid_subset_size=3, is_splits=2, prc_neighborhood=2, dc_nearest_k=3)
    calc = V.ValidationMetrics("cuda", config["clip_model_name"], extra_metrics=("dc", "kid", "is", "prc"), **weights, **small)
    assert calc.fid_metric.inception is calc.inception is calc.kid_metric.inception is calc.prc_metric.inception
    calls = []
    tower = calc.inception.forward
    calc.inception.forward = lambda x: (calls.append(x.shape[0]), tower(x))[1]
    results, overall, seen = run(setup, tmp_path, "device", metrics=calc)
    assert calls == [2, 2, 2, 2]                                        # one tower call per side per batch, whatever the number of metrics
    orows = read_csv(tmp_path / "overall_metrics.csv")
    assert [r[0] for r in orows[1:]] == REFERENCE_ROWS + EXTRA_ROWS == list(overall.keys())
    w = weights["inception_weights"]
    kw = dict(weights=w, normalize=True)
    fid, kid = FrechetInceptionDistance(**kw), KernelInceptionDistance(subsets=5, subset_size=3, **kw)
    isc, prc, dc = InceptionScore(splits=2, **kw), PrecisionRecall(neighborhood=2, **kw), DensityCoverage(nearest_k=3, **kw)
    for _, gen, tgt, _ in seen:
        g01, t01 = (gen.clamp(-1, 1) + 1) / 2.0, (tgt.clamp(-1, 1) + 1) / 2.0
        for m in (fid, kid, prc, dc):
            m.update(g01, real=False)
            m.update(t01, real=True)
        isc.update(g01)
    assert overall["fid"] == fid.compute().item()
    assert [overall[k] for k in ("precision", "recall", "f_score")] == [float(v) for v in prc.compute()]
    assert [overall[k] for k in ("density", "coverage")] == [float(v) for v in dc.compute()]
    torch.manual_seed(9)                       # KID draws its subsets and the Inception score its permutation from torch's generator
    shared = calc.compute_extras()
    torch.manual_seed(9)
    assert [shared["kid_mean"], shared["kid_std"]] == [float(v) for v in kid.compute()]
    want_is = [float(v) for v in isc.compute()]
    assert [shared["inception_score_mean"], shared["inception_score_std"]] == want_is
    assert list(shared) == EXTRA_ROWS
