"""Drop-in for the reference's src/data/objaverse_dataset.py (imported by val.py:24): ``ObjaverseDataset`` with the reference's
constructor, split, pair cache and sample dict, plus ``frontend="device"`` and its ``DeviceCollate`` (mvd_amd/dataset.py).
``ObjaverseDataModule`` (Lightning) is not provided."""
from mvd_amd.dataset import DeviceCollate, ObjaverseDataset  # noqa: F401
