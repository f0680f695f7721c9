"""The shared Inception tower of ``ValidationMetrics`` feeds the extra metrics also when FID itself could not be built.  (The loader's
worker processes are tested without a GPU, tests/test_dataset_workers_cpu.py: they never touch the device, and the main-process
collate they feed is the path every test of tests/test_val_gpu.py runs.)"""
import pytest
import torch

from mvd_amd import val as V
from test_val_gpu import setup  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu


def test_extras_are_fed_without_fid(setup):        # noqa: F811
    config, _, weights, _ = setup
    calc = V.ValidationMetrics("cuda", config["clip_model_name"], extra_metrics=("kid", "prc"), kid_subsets=3, kid_subset_size=2,
                               prc_neighborhood=1, **weights)
    calc.fid_metric = None                             # as if FID had failed to build
    g = torch.Generator().manual_seed(4)
    gen, tgt = (torch.rand(2, 3, 64, 64, generator=g).cuda() * 2 - 1 for _ in range(2))
    calc.calculate_metrics(gen, tgt, None)
    assert len(calc.kid_metric.fake_features) == len(calc.kid_metric.real_features) == 1
    assert len(calc.prc_metric.fake_features) == len(calc.prc_metric.real_features) == 1
    assert calc.compute_fid() == 0.0
    extras = calc.compute_extras()
    assert list(extras) == ["kid_mean", "kid_std", "precision", "recall", "f_score"] and 0.0 <= extras["precision"] <= 1.0
