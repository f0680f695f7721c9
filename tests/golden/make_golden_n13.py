"""Writes the N13 fixtures.  Run from the repository root, on a machine that has Pillow and a checkout of the reference project:

    python tests/golden/make_golden_n13.py [--reference DIR]

  n13_frontend.npz   live PIL's composite-on-white + LANCZOS output for the seeded inputs of tests/imageio_ref.py (every case and
                     image kind as RGBA, the random kind also as RGB), with the Pillow version inside -- the GPU machine needs no PIL
  n13_dataset.json   (with --reference) split, pair list, prompts and cache file name of the reference's own ObjaverseDataset on the
                     synthetic tree of tests/n13_tree.py, paths relative to the tree; and calculate_overall_metrics / save_results of
                     the reference's val.py on the hand-made batch list of tests/n13_tree.py
The reference modules are imported with stub modules for the third-party packages they import but these functions do not use.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import imageio_ref as R  # noqa: E402


def golden_keys():
    for case in R.CASES:
        for kind in R.KINDS:
            for ch in ((4, 3) if kind == "random" else (4,)):
                yield case, kind, ch, f"{R.case_name(case)}_{kind}_c{ch}"


def write_frontend(path):
    import PIL
    out = {"pil_version": np.array(PIL.__version__)}
    for case, kind, ch, key in golden_keys():
        out[key] = R.pil_frontend(R.make_input(case, kind, ch, 1), case[2], case[3])
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(ref_dir):
    """the reference's dataset module and val.py, with stubs for what does not import here"""
    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return self
        def __getattr__(self, n): return _Any()
    _stub("icecream", ic=lambda *a, **k: None)
    _stub("pytorch_lightning", LightningDataModule=object)
    for name in ("matplotlib", "matplotlib.pyplot", "lovely_tensors", "lpips", "pytorch_msssim", "torchmetrics", "torchmetrics.image",
                 "torchmetrics.multimodal", "tqdm", "src.models.mvd_unet", "src.training.losses"):
        if name in sys.modules:
            continue
        try:
            if not name.startswith("src."):
                importlib.import_module(name)
                continue
        except Exception:
            pass
        _stub(name, monkey_patch=lambda: None, SSIM=_Any, FrechetInceptionDistance=_Any, PeakSignalNoiseRatio=_Any, CLIPScore=_Any,
              tqdm=lambda it, **k: it, create_mvd_pipeline=_Any, PerceptualLoss=_Any, LPIPS=_Any)
    sys.path.insert(0, ref_dir)
    for m in [k for k in sys.modules if k == "src" or (k.startswith("src.") and not isinstance(sys.modules[k], types.ModuleType))]:
        del sys.modules[m]
    ds = importlib.import_module("src.data.objaverse_dataset")
    try:
        val = importlib.import_module("val")
    except Exception as e:      # noqa: BLE001
        print("val.py did not import even with stubs:", repr(e))
        val = None
    return ds, val


def write_dataset(path, ref_dir):
    import n13_tree as T
    ds_mod, val_mod = import_reference(ref_dir)
    out = {"datasets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        root = T.build_tree(tmp)
        for name, kw in T.DATASET_CONFIGS.items():
            d = ds_mod.ObjaverseDataset(data_root=str(root), **kw)
            rel = lambda p: os.path.relpath(p, root)      # noqa: E731
            caches = sorted(f for f in os.listdir(root) if f.endswith(".json"))
            out["datasets"][name] = {
                "zip_files": [rel(z) for z in d.zip_files],
                "view_pairs": [{**p, "zip_path": rel(p["zip_path"])} for p in d.view_pairs],
                "len": len(d),
            }
            for f in caches:
                os.remove(os.path.join(root, f))
    if val_mod is not None:
        batches, results = T.val_batches()
        overall = val_mod.calculate_overall_metrics(batches, T.VAL_FID)
        with tempfile.TemporaryDirectory() as tmp:
            from pathlib import Path
            val_mod.save_results(results, overall, Path(tmp))
            out["val"] = {"overall_keys": list(overall.keys()), "overall": {k: float(v) for k, v in overall.items()},
                          "validation_results_csv": open(os.path.join(tmp, "validation_results.csv"), newline="").read(),
                          "overall_metrics_csv": open(os.path.join(tmp, "overall_metrics.csv"), newline="").read(),
                          "empty": val_mod.calculate_overall_metrics([], 1.0)}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference project (for n13_dataset.json)")
    a = ap.parse_args()
    write_frontend(os.path.join(HERE, "n13_frontend.npz"))
    if a.reference:
        write_dataset(os.path.join(HERE, "n13_dataset.json"), a.reference)
