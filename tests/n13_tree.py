"""The seeded synthetic Objaverse tree and the hand-made validation batches of the N13 tests (and of tests/golden/make_golden_n13.py,
which records what the reference's own classes make of them).

``build_tree(dir)`` writes ``dir/renders_final/<uid>.zip`` for 14 objects: RGBA and RGB renders of several sizes, ``.npy`` cameras,
some with ``prompt.txt``; one object with more images than cameras, one with a single view, one whose renders are greyscale."""
from __future__ import annotations

import io
import zipfile
from pathlib import Path

import numpy as np

# name -> keyword arguments of ObjaverseDataset beyond data_root
DATASET_CONFIGS = {
    "train": dict(split="train"),
    "val": dict(split="val"),
    "test": dict(split="test", max_views_per_object=3),
    "train_max5_seed7": dict(split="train", dataset_samples=5, seed=7),
    "all_3views": dict(split="train", split_ratio=(1.0, 0.0, 0.0), max_views_per_object=3),
    "thirds": dict(split="val", split_ratio=(0.5, 0.25, 0.25), max_views_per_object=2, seed=3),
}

N_OBJECTS = 14


def _png(rng, mode, h, w) -> bytes:
    from PIL import Image
    ch = {"RGBA": 4, "RGB": 3, "L": 1}[mode]
    a = rng.randint(0, 256, (h, w, ch)).astype(np.uint8)
    if mode == "RGBA":
        a[..., 3] = np.where(rng.rand(h, w) < 0.5, 255, a[..., 3])        # half opaque, the rest any alpha
    buf = io.BytesIO()
    Image.fromarray(a[..., 0] if mode == "L" else a, mode).save(buf, format="PNG")
    return buf.getvalue()


def build_tree(directory) -> Path:
    root = Path(directory) / "objaverse"
    renders = root / "renders_final"
    renders.mkdir(parents=True, exist_ok=True)
    rng = np.random.RandomState(1313)
    for i in range(N_OBJECTS):
        uid = f"obj{i:02d}{'abcdefghijklmn'[i]}"
        views = [5, 4, 3, 6, 2, 4, 1, 4, 3, 5, 4, 2, 3, 4][i]
        mode = "L" if i == 9 else ("RGB" if i % 3 == 1 else "RGBA")
        h, w = [(48, 48), (40, 56), (32, 32), (64, 48)][i % 4]
        with zipfile.ZipFile(renders / f"{uid}.zip", "w") as z:
            for v in range(views):
                z.writestr(f"{uid}/{v:03d}.png", _png(rng, mode, h, w))
                if not (i == 3 and v == views - 1):               # object 3: one camera short
                    cam = np.eye(4)
                    cam[:3, :] = rng.randn(3, 4)
                    buf = io.BytesIO()
                    np.save(buf, cam)
                    z.writestr(f"{uid}/{v:03d}.npy", buf.getvalue())
            if i % 2 == 0:
                z.writestr(f"{uid}/prompt.txt", f"  a synthetic object number {i}, étude\n")
    return root


# ---------------------------------------------------------------- validation: a hand-made batch list
VAL_FID = 12.5
_KEYS = ("psnr", "ssim", "perceptual_loss", "lpips", "clip_score")


def val_batches():
    """(batch_metrics, all_results) shaped as run_validation builds them: zeros, a negative value and a missing CLIP score exercise
    the `> 0` filters"""
    rows = [(21.5, 0.81, 0.40, 0.22, 27.0, 1.25, 2), (19.25, 0.0, 0.55, 0.31, 0.0, 1.5, 2), (23.0, 0.77, -0.1, 0.0, 31.5, 0.75, 1),
            (20.125, 0.9, 0.35, 0.18, 29.25, 1.0, 2)]
    batches, results = [], []
    for b, row in enumerate(rows):
        d = dict(zip(_KEYS, row[:5]))
        d["batch_inference_time_seconds"] = row[5]
        d["num_samples_in_batch"] = row[6]
        batches.append(d)
        for i in range(row[6]):
            s = {"object_uid": f"uid{b}_{i}", "prompt": f"prompt, with a comma {b}" if i else DEFAULT_PROMPT, "inference_time_seconds": row[5] / row[6]}
            for k in _KEYS[:4]:
                s[k] = d[k] + 0.125 * i
            s["clip_score"] = d["clip_score"]
            s["batch_inference_time_seconds"] = row[5]
            s["num_samples_in_batch"] = row[6]
            results.append(s)
    return batches, results


DEFAULT_PROMPT = "3D object"
