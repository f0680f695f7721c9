"""``mvd_amd.val``'s aggregation and CSV writers against the reference's own functions on the hand-made batch list of
tests/n13_tree.py (tests/golden/n13_dataset.json, section "val", recorded by tests/golden/make_golden_n13.py: the reference's val.py
imports with stub modules for its third-party packages, so nothing is restated); the drop-in shim; the configuration reader."""
import json
import os
import sys

import pytest

import n13_tree as T
from mvd_amd import val as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "n13_dataset.json")) as f:
        return json.load(f)["val"]


def test_overall_metrics_are_the_references(golden):
    batches, _ = T.val_batches()
    got = V.calculate_overall_metrics(batches, T.VAL_FID)
    assert list(got.keys()) == golden["overall_keys"]                 # the rows and their order
    for k, v in got.items():
        assert float(v) == golden["overall"][k], k                    # numpy's own mean / std / min / max: the same bits
    assert "ssim_mean" in got and got["ssim_min"] == 0.77             # the 0.0 batch is left out (`> 0`)
    assert got["perceptual_loss_min"] == 0.35 and got["lpips_min"] == 0.18
    assert got["total_samples_processed_in_inference"] == 7
    assert V.calculate_overall_metrics([], 1.0) == golden["empty"] == {}


def test_a_metric_without_positive_values_has_no_rows_and_no_times_gives_zero_rows():
    got = V.calculate_overall_metrics([{"psnr": 0.0, "ssim": -1.0, "clip_score": 0.0}], 3.0)
    assert list(got) == ["fid", "mean_batch_inference_time_seconds", "total_inference_duration_seconds", "total_samples_processed_in_inference",
                         "avg_per_sample_inference_time_seconds"]
    assert got["fid"] == 3.0 and got["avg_per_sample_inference_time_seconds"] == 0.0


def test_csv_files_are_the_references_byte_for_byte(golden, tmp_path):
    batches, results = T.val_batches()
    overall = V.calculate_overall_metrics(batches, T.VAL_FID)
    V.save_results(results, overall, tmp_path)
    assert open(tmp_path / "validation_results.csv", newline="").read() == golden["validation_results_csv"]
    assert open(tmp_path / "overall_metrics.csv", newline="").read() == golden["overall_metrics_csv"]
    header = golden["validation_results_csv"].splitlines()[0]
    assert header == "object_uid,prompt,inference_time_seconds,psnr,ssim,perceptual_loss,lpips,clip_score,batch_inference_time_seconds,num_samples_in_batch"


def test_no_results_writes_the_overall_file_alone(tmp_path):
    V.save_results([], {"fid": 1.5}, tmp_path)
    assert not (tmp_path / "validation_results.csv").exists()
    assert open(tmp_path / "overall_metrics.csv", newline="").read() == "Metric,Value\r\nfid,1.5\r\n"


def test_load_config_and_cli_errors(tmp_path, capsys):
    pytest.importorskip("yaml")
    with pytest.raises(FileNotFoundError):
        V.load_config(str(tmp_path / "none.yaml"))
    p = tmp_path / "c.yaml"
    p.write_text("architecture: fake-org/tiny\nimage_size: [64, 48]\nbatch_size: 2\n")
    assert V.load_config(str(p)) == {"architecture": "fake-org/tiny", "image_size": [64, 48], "batch_size": 2}
    assert V.main(["--ckpt", "x.ckpt", "--dataset-path", str(tmp_path), "--config", str(tmp_path / "none.yaml"), "--output-dir", str(tmp_path / "o")]) == 1
    assert V.main(["--ckpt", str(tmp_path / "x.ckpt"), "--dataset-path", str(tmp_path), "--config", str(p), "--output-dir", str(tmp_path / "o")]) == 1
    with pytest.raises(SystemExit):
        V.main(["--dataset-path", "x"])


def test_unknown_extra_metric_is_refused():
    from mvd_amd._lib import MvdError
    with pytest.raises(MvdError, match="extra_metrics"):
        V.ValidationMetrics("cpu", extra_metrics=("kid", "fidelity"))


def test_shim_exports_the_dataset():
    p = os.path.join(ROOT, "integration")
    sys.path.insert(0, p)
    saved = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]}
    try:
        from src.data.objaverse_dataset import DeviceCollate, ObjaverseDataset
        from mvd_amd import dataset as D
        assert ObjaverseDataset is D.ObjaverseDataset and DeviceCollate is D.DeviceCollate
    finally:
        sys.path.remove(p)
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
