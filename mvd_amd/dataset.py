"""``ObjaverseDataset`` of the reference (src/data/objaverse_dataset.py:23-337) without Lightning, with a second mode in which the
image work runs on the device.

The constructor, the attributes, the split, the pair list, the cache file and the sample dict are the reference's, so a pair cache
written by either side is read by the other: ``random.Random(seed)`` shuffles the sorted zip list, ``int()`` bounds cut it,
``rng.sample`` draws the views of every object, and the cache is named after the md5 of the joined sorted paths of the split.  The
reference's quirks are kept on purpose.

``frontend="host"`` (default): PIL composites, resizes and the sample holds the reference's float tensors.
``frontend="device"``: the sample holds the decoded uint8 arrays as they are; the ``DataLoader``'s workers hand them back untouched
(``collate_fn=raw_collate``) and ``DeviceCollate``, in the main process, copies a batch of them to the GPU and runs
``image_frontend.composite_resize`` there -- the batch equals the host mode's bit for bit, and the host is left with the inflate
alone.  ``ObjaverseDataModule`` (Lightning) is not built.
"""
from __future__ import annotations

import glob
import hashlib
import io
import json
import logging
import os
import random
import zipfile
from pathlib import Path
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from ._lib import MvdError

logger = logging.getLogger(__name__)

DEFAULT_PROMPT = "3D object"      # what an object without prompt.txt is called
MAX_RETRIES = 3


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise MvdError("ObjaverseDataset decodes PNG renders with the 'Pillow' package (PIL), which is not installed") from e
    return Image


class ObjaverseDataset(Dataset):
    def __init__(self, data_root: str, split: str = "train", split_ratio: Tuple[float, float, float] = (0.8, 0.1, 0.1), transform=None,
                 target_size: Tuple[int, int] = (256, 256), max_views_per_object: int = 4, seed: int = 42,
                 dataset_samples: Optional[int] = None, frontend: str = "host"):
        super().__init__()
        if frontend not in ("host", "device"):
            raise MvdError(f"ObjaverseDataset: frontend={frontend!r} (\"host\" or \"device\")")
        if frontend == "device" and transform is not None:
            raise MvdError("ObjaverseDataset: a PIL transform needs frontend=\"host\" (the device mode hands out raw arrays)")
        self.frontend = frontend
        self.data_root = Path(data_root)
        self.split = split
        self._split_ratio_arg = split_ratio
        self.transform = transform
        self.target_size = target_size
        self.max_views_per_object = max_views_per_object
        self.dataset_samples = dataset_samples
        self.seed = seed
        self.rng = random.Random(self.seed)
        self._initial_all_zip_files_on_disk = self._zips_on_disk()
        logger.info("found %d object zip files under %s", len(self._initial_all_zip_files_on_disk), self.data_root / "renders_final")
        self._split_dataset(self._initial_all_zip_files_on_disk, self._split_ratio_arg)
        self.view_pairs = []
        self._build_view_pairs()

    def _zips_on_disk(self):
        return sorted(glob.glob(str(self.data_root / "renders_final" / "*.zip")))

    # ------------------------------------------------------------------ split
    def _split_dataset(self, all_zips, split_ratio) -> None:
        assert sum(split_ratio) == 1.0, "Split ratios must sum to 1.0"
        shuffled = list(all_zips)
        self.rng.shuffle(shuffled)
        train_end = int(len(shuffled) * split_ratio[0])
        val_end = train_end + int(len(shuffled) * split_ratio[1])
        if self.split == "train":
            self.zip_files = shuffled[:train_end]
        elif self.split == "val":
            self.zip_files = shuffled[train_end:val_end]
        elif self.split == "test":
            self.zip_files = shuffled[val_end:]
        else:
            raise ValueError(f"Unknown split: {self.split}")
        # names the pair cache of exactly this split of exactly these files
        self.zip_files_hash = hashlib.md5("".join(sorted(self.zip_files)).encode()).hexdigest()
        logger.info("%d objects in the %s split (hash %s)", len(self.zip_files), self.split, self.zip_files_hash)

    # ------------------------------------------------------------------ pairs
    def cache_path(self) -> Path:
        suffix = f"_max{self.dataset_samples}" if self.dataset_samples is not None else "_all"
        return self.data_root / f"objaverse_{self.split}_pairs_cache_{self.zip_files_hash}{suffix}.json"

    def _full(self) -> bool:
        return self.dataset_samples is not None and len(self.view_pairs) >= self.dataset_samples

    def _build_view_pairs(self) -> None:
        cache = self.cache_path()
        if cache.exists():
            try:
                with open(cache, "r") as f:
                    self.view_pairs = json.load(f)
                logger.info("%d view pairs from the cache %s", len(self.view_pairs), cache)
                return
            except Exception as e:  # noqa: BLE001
                logger.warning("cache file %s did not load (%s); rebuilding", cache, e)
        for zip_path in self.zip_files:
            uid = Path(zip_path).stem
            try:
                with zipfile.ZipFile(zip_path, "r") as z:
                    names = z.namelist()
                    pngs = sorted(n for n in names if n.endswith(".png"))
                    npys = sorted(n for n in names if n.endswith(".npy"))
                    prompts = [n for n in names if n == f"{uid}/prompt.txt"]
                    if len(pngs) != len(npys) or not pngs:
                        logger.warning("skipping %s: %d images, %d camera files", uid, len(pngs), len(npys))
                        continue
                    prompt = DEFAULT_PROMPT
                    if prompts:
                        with z.open(prompts[0]) as f:
                            prompt = f.read().decode("utf-8").strip()
                    num_views = min(len(pngs), self.max_views_per_object)
                    if num_views < 2:
                        logger.warning("skipping %s: %d view", uid, num_views)
                        continue
                    views = self.rng.sample(range(len(pngs)), num_views)
                    for i, s in enumerate(views):
                        for t in views[i + 1:]:
                            self.view_pairs.append({"zip_path": zip_path, "object_uid": uid, "prompt": prompt, "source_image": pngs[s],
                                                    "source_camera": npys[s], "target_image": pngs[t], "target_camera": npys[t]})
            except Exception as e:  # noqa: BLE001
                logger.error("error processing %s: %s", zip_path, e)
                continue
            if self._full():      # an object's pairs are never cut: the list may end above dataset_samples
                break
        try:
            with open(cache, "w") as f:
                json.dump(self.view_pairs, f)
        except Exception as e:  # noqa: BLE001
            logger.error("could not write the cache file %s: %s", cache, e)
        logger.info("%d view pairs for the %s split", len(self.view_pairs), self.split)

    def __len__(self) -> int:
        return len(self.view_pairs)

    # ------------------------------------------------------------------ samples
    def __getitem__(self, idx: int) -> Dict[str, Any]:
        # the reference's retry: a pair whose zip is gone or broken is popped from the list (the dataset shrinks) and the next
        # index is tried, three times in all
        last = None
        for _ in range(MAX_RETRIES):
            try:
                pair = self.view_pairs[idx]
                zip_path = pair["zip_path"]
                if not os.path.exists(zip_path):
                    self.view_pairs.pop(idx)
                    idx = (idx + 1) % len(self.view_pairs)
                    continue
                with zipfile.ZipFile(zip_path, "r") as z:
                    src_img = self._load_image(z, pair["source_image"])
                    src_cam = self._load_camera(z, pair["source_camera"])
                    tgt_img = self._load_image(z, pair["target_image"])
                    tgt_cam = self._load_camera(z, pair["target_camera"])
                break
            except (FileNotFoundError, zipfile.BadZipFile, KeyError) as e:
                last = e
                self.view_pairs.pop(idx)
                idx = (idx + 1) % len(self.view_pairs)
        else:
            raise RuntimeError(f"Failed to load valid sample after {MAX_RETRIES} attempts. Last error: {last}")
        if self.frontend == "device":
            src_t, tgt_t = torch.from_numpy(src_img), torch.from_numpy(tgt_img)
        else:
            if self.transform:
                src_img, tgt_img = self.transform(src_img), self.transform(tgt_img)
            src_t = torch.from_numpy(np.array(src_img)).permute(2, 0, 1).float() / 127.5 - 1.0
            tgt_t = torch.from_numpy(np.array(tgt_img)).permute(2, 0, 1).float() / 127.5 - 1.0
        return {"object_uid": pair["object_uid"], "prompt": pair["prompt"], "source_image": src_t, "target_image": tgt_t,
                "source_camera": torch.from_numpy(src_cam).float(), "target_camera": torch.from_numpy(tgt_cam).float()}

    def _load_image(self, z: zipfile.ZipFile, name: str):
        """host mode: the PIL image, composited on white and LANCZOS-resized to target_size; device mode: the decoded (h, w, 3 | 4)
        uint8 array, untouched"""
        Image = _pil()
        with z.open(name) as f:
            img = Image.open(io.BytesIO(f.read()))
            if self.frontend == "device":
                if img.mode not in ("RGB", "RGBA"):
                    img = img.convert("RGB")
                return np.array(img)
            if img.mode == "RGBA":
                img = Image.alpha_composite(Image.new("RGBA", img.size, (255, 255, 255, 255)), img)
            img = img.convert("RGB")
            if img.size != self.target_size:
                img = img.resize(self.target_size, Image.Resampling.LANCZOS)
            return img

    def _load_camera(self, z: zipfile.ZipFile, name: str) -> np.ndarray:
        with z.open(name) as f:
            return np.load(io.BytesIO(f.read()))

    # ------------------------------------------------------------------ resuming
    def state_dict(self):
        return {"rng_state": self.rng.getstate()}

    def load_state_dict(self, state_dict):
        """restores the generator and re-runs the split and the pair building from it, on the zips that are on disk now"""
        self.rng.setstate(state_dict["rng_state"])
        now = self._zips_on_disk()
        if len(now) != len(self._initial_all_zip_files_on_disk):
            logger.warning("the number of zip files changed: %d at construction, %d now", len(self._initial_all_zip_files_on_disk), len(now))
            self._initial_all_zip_files_on_disk = now
        self._split_dataset(self._initial_all_zip_files_on_disk, self._split_ratio_arg)
        self.view_pairs = []
        self._build_view_pairs()


def raw_collate(samples):
    """``collate_fn`` for the ``DataLoader``'s WORKER processes over a device-mode dataset: the samples as they are, a list of dicts
    with uint8 arrays.  The workers only inflate; ``DeviceCollate`` then runs on the list in the main process."""
    return list(samples)


class DeviceCollate:
    """Turns a list of samples of an ``ObjaverseDataset(frontend="device")`` into the batch dict: groups the raw images by size and
    channel count, copies each group to ``device`` (through pinned memory when asked) and runs ``composite_resize``; the batch
    equals the host mode's default-collated dict bit for bit, with the two image tensors on the device.

    It belongs in the process that owns the GPU.  With ``num_workers=0`` it may be the ``DataLoader``'s ``collate_fn``; with worker
    processes give the loader ``collate_fn=raw_collate`` and call this on what the loader yields --

        collate = DeviceCollate("cuda", (512, 512))
        for samples in DataLoader(ds, batch_size=8, num_workers=8, collate_fn=raw_collate):
            batch = collate(samples)

    -- called inside a worker it raises ``MvdError`` (a forked worker cannot use the parent's GPU context, and one context per
    worker is not wanted).  A horizontal downscale above about 9 (1024 wide to under 108) is refused by the kernel: use the host
    mode for such sizes."""

    IMAGE_KEYS = ("source_image", "target_image")

    def __init__(self, device, target_size: Tuple[int, int], pin: bool = True):
        self.device = torch.device(device)
        self.target_size = (int(target_size[0]), int(target_size[1]))
        self.pin = pin

    def _images(self, raws) -> torch.Tensor:
        from .image_frontend import composite_resize
        groups: Dict[tuple, list] = {}
        for i, r in enumerate(raws):
            groups.setdefault(tuple(r.shape), []).append(i)
        pieces = [None] * len(raws)
        for idxs in groups.values():
            stack = torch.stack([raws[i] for i in idxs])
            if self.pin:
                stack = stack.pin_memory()
            res = composite_resize(stack.to(self.device, non_blocking=self.pin), self.target_size, out="float")
            if len(groups) == 1:
                return res                      # the usual case: every render has one size
            for j, i in enumerate(idxs):
                pieces[i] = res[j]
        return torch.stack(pieces)              # sample order, no index tensor from the host

    def __call__(self, samples):
        from torch.utils.data import default_collate, get_worker_info
        if get_worker_info() is not None:
            raise MvdError("DeviceCollate was called inside a DataLoader worker process; it belongs in the main process: give the "
                           "DataLoader collate_fn=mvd_amd.dataset.raw_collate and call DeviceCollate on the lists it yields")
        batch = {}
        for k in samples[0]:
            vals = [s[k] for s in samples]
            batch[k] = self._images(vals) if k in self.IMAGE_KEYS else default_collate(vals)
        return batch
