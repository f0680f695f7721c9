"""The device-mode loader with worker processes, without a GPU: the workers of a ``DataLoader`` over
``ObjaverseDataset(frontend="device")`` hand back the raw uint8 arrays (``collate_fn=raw_collate``) and never touch the device;
``DeviceCollate`` refuses to run inside a worker; ``run_validation`` builds its loader that way for any ``num_workers``."""
import pytest
import torch
from torch.utils.data import DataLoader

import n13_tree as T

pytest.importorskip("PIL")

from mvd_amd.dataset import DeviceCollate, ObjaverseDataset, raw_collate  # noqa: E402


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    root = T.build_tree(tmp_path_factory.mktemp("workers"))
    return ObjaverseDataset(data_root=str(root), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(32, 32), max_views_per_object=2,
                            frontend="device")


def _cuda_untouched(_worker_id):
    assert not torch.cuda.is_initialized()


class _Probe:
    """raw_collate that also reports whether the worker has initialised the GPU runtime"""

    def __call__(self, samples):
        return raw_collate(samples), torch.cuda.is_initialized(), torch.utils.data.get_worker_info().id


def test_workers_hand_back_raw_uint8_arrays_and_never_touch_the_device(ds):
    direct = [ds[i] for i in range(len(ds))]
    seen, workers = [], set()
    for samples, cuda_up, wid in DataLoader(ds, batch_size=3, shuffle=False, num_workers=2, collate_fn=_Probe(), worker_init_fn=_cuda_untouched):
        assert isinstance(samples, list) and not cuda_up
        workers.add(wid)
        seen.extend(samples)
    assert workers == {0, 1} and len(seen) == len(direct) > 6
    for got, want in zip(seen, direct):
        assert list(got) == list(want) and got["object_uid"] == want["object_uid"] and got["prompt"] == want["prompt"]
        for k in ("source_image", "target_image"):
            assert got[k].dtype == torch.uint8 and not got[k].is_cuda and got[k].dim() == 3 and got[k].shape[-1] in (3, 4)
            assert torch.equal(got[k], want[k])
        assert torch.equal(got["source_camera"], want["source_camera"])


def test_device_collate_refuses_to_run_in_a_worker(ds):
    loader = DataLoader(ds, batch_size=2, num_workers=2, collate_fn=DeviceCollate("cuda", (32, 32)))
    with pytest.raises(Exception, match="main process"):
        next(iter(loader))


def test_run_validation_collates_in_the_main_process(ds, tmp_path, monkeypatch):
    """run_validation's loader for a device-mode dataset: raw_collate in the workers, DeviceCollate on the yielded list here"""
    from mvd_amd import dataset as D
    from mvd_amd import val as V
    calls = []

    class Recording(D.DeviceCollate):
        def __call__(self, samples):
            assert torch.utils.data.get_worker_info() is None
            calls.append([s["object_uid"] for s in samples])
            assert all(s["source_image"].dtype == torch.uint8 for s in samples)
            raise RuntimeError("stop here: no GPU in this test")
    monkeypatch.setattr(D, "DeviceCollate", Recording)

    class Metrics:
        extra_metrics = ()

        def compute_fid(self):
            return 0.0
    config = dict(batch_size=4, num_workers=2)
    results, overall = V.run_validation(None, ds, config, "cpu", tmp_path, metrics=Metrics())
    assert results == [] and overall == {}                      # every batch raised in the collate and was skipped, as logged
    assert len(calls) == (len(ds) + 3) // 4 and sum(len(c) for c in calls) == len(ds)
    assert [u for c in calls for u in c] == [p["object_uid"] for p in ds.view_pairs]
