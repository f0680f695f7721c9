"""``mvd_amd.dataset.ObjaverseDataset`` against what the reference's own class made of the same synthetic tree (tests/n13_tree.py):
tests/golden/n13_dataset.json, recorded by tests/golden/make_golden_n13.py with paths relative to the tree."""
import hashlib
import json
import os
import zipfile

import numpy as np
import pytest
import torch

import n13_tree as T

pytest.importorskip("PIL")

from mvd_amd.dataset import ObjaverseDataset  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n13_dataset.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["datasets"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return T.build_tree(tmp_path_factory.mktemp("n13"))


def _clear_caches(root):
    for f in os.listdir(root):
        if f.endswith(".json"):
            os.remove(os.path.join(root, f))


@pytest.mark.parametrize("name", sorted(T.DATASET_CONFIGS))
def test_split_pairs_prompts_and_cache_name_are_the_references(tree, golden, name):
    _clear_caches(tree)
    kw = T.DATASET_CONFIGS[name]
    d = ObjaverseDataset(data_root=str(tree), **kw)
    g = golden[name]
    rel = lambda p: os.path.relpath(p, tree)      # noqa: E731
    assert [rel(z) for z in d.zip_files] == g["zip_files"]
    got = [{**p, "zip_path": rel(p["zip_path"])} for p in d.view_pairs]
    assert got == g["view_pairs"] and len(d) == g["len"]
    assert [list(p.keys()) for p in got] == [list(p.keys()) for p in g["view_pairs"]]          # the cache file's key order too
    # the cache: the reference's name, from the md5 of the joined sorted absolute paths of the split
    suffix = f"_max{kw['dataset_samples']}" if kw.get("dataset_samples") is not None else "_all"
    md5 = hashlib.md5("".join(sorted(d.zip_files)).encode()).hexdigest()
    assert d.zip_files_hash == md5
    cache = tree / f"objaverse_{kw['split']}_pairs_cache_{md5}{suffix}.json"
    assert d.cache_path() == cache and cache.exists()
    with open(cache) as f:
        assert f.read() == json.dumps(d.view_pairs)
    _clear_caches(tree)


def test_golden_covers_the_quirks(golden):
    allp = golden["all_3views"]["view_pairs"]
    uids = {p["object_uid"] for p in allp}
    assert "obj03d" not in uids and "obj06g" not in uids          # mismatched files; a single view
    assert {p["prompt"] for p in allp if p["object_uid"] == "obj01b"} == {"3D object"}
    assert any(p["prompt"].endswith("étude") for p in allp)       # stripped, utf-8
    assert golden["train_max5_seed7"]["len"] >= 5                   # the early stop never cuts an object's pairs
    assert golden["train_max5_seed7"]["len"] < golden["train"]["len"]


def test_a_cache_written_by_the_other_side_is_read(tree, golden):
    """the reference's cache content (its pair list, absolute paths) under the reference's name is taken as it is, not rebuilt"""
    _clear_caches(tree)
    d = ObjaverseDataset(data_root=str(tree), split="test", max_views_per_object=3)
    cache = d.cache_path()
    theirs = [{**p, "zip_path": str(tree / p["zip_path"])} for p in golden["test"]["view_pairs"]]
    assert d.view_pairs == theirs
    marked = [dict(p, prompt="from the cache") for p in theirs[:2]]
    with open(cache, "w") as f:
        json.dump(marked, f)
    d2 = ObjaverseDataset(data_root=str(tree), split="test", max_views_per_object=3)
    assert d2.view_pairs == marked and len(d2) == 2
    with open(cache, "w") as f:
        f.write("{ not json")
    d3 = ObjaverseDataset(data_root=str(tree), split="test", max_views_per_object=3)          # a broken cache is rebuilt
    assert d3.view_pairs == theirs
    _clear_caches(tree)


def test_state_dict_round_trip(tree):
    _clear_caches(tree)
    d = ObjaverseDataset(data_root=str(tree), split="train", seed=11)
    state = d.state_dict()
    assert list(state) == ["rng_state"]
    _clear_caches(tree)
    first_zips, first_pairs = list(d.zip_files), list(d.view_pairs)
    d.load_state_dict(state)             # the generator has moved on: the split is drawn again from the restored state
    again_zips, again_pairs = list(d.zip_files), list(d.view_pairs)
    _clear_caches(tree)
    d.load_state_dict(state)
    assert d.zip_files == again_zips and d.view_pairs == again_pairs
    assert len(again_zips) == len(first_zips)
    e = ObjaverseDataset(data_root=str(tree), split="train", seed=11)
    assert e.zip_files == first_zips
    _clear_caches(tree)


def test_host_sample_is_pil_composite_lanczos(tree):
    import io
    from PIL import Image
    _clear_caches(tree)
    d = ObjaverseDataset(data_root=str(tree), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(40, 24), max_views_per_object=2)
    seen = set()
    for i in range(len(d)):
        s = d[i]
        p = d.view_pairs[i]
        assert list(s) == ["object_uid", "prompt", "source_image", "target_image", "source_camera", "target_camera"]
        assert s["object_uid"] == p["object_uid"] and s["prompt"] == p["prompt"]
        with zipfile.ZipFile(p["zip_path"]) as z:
            for side in ("source", "target"):
                im = Image.open(io.BytesIO(z.read(p[f"{side}_image"])))
                seen.add(im.mode)
                if im.mode == "RGBA":
                    im = Image.alpha_composite(Image.new("RGBA", im.size, (255, 255, 255, 255)), im)
                im = im.convert("RGB").resize((40, 24), Image.Resampling.LANCZOS)
                want = torch.from_numpy(np.asarray(im, dtype=np.float32) / 127.5 - 1.0).permute(2, 0, 1)
                assert s[f"{side}_image"].shape == (3, 24, 40) and torch.equal(s[f"{side}_image"], want)
                cam = np.load(io.BytesIO(z.read(p[f"{side}_camera"])))
                assert s[f"{side}_camera"].dtype == torch.float32 and torch.equal(s[f"{side}_camera"], torch.from_numpy(cam).float())
    assert seen == {"RGBA", "RGB", "L"}
    _clear_caches(tree)


def test_device_mode_hands_out_the_decoded_arrays(tree):
    import io
    from PIL import Image
    from mvd_amd._lib import MvdError
    _clear_caches(tree)
    kw = dict(data_root=str(tree), split="train", split_ratio=(1.0, 0.0, 0.0), max_views_per_object=2)
    d = ObjaverseDataset(frontend="device", **kw)
    for i in (0, len(d) // 2, len(d) - 1):
        s, p = d[i], d.view_pairs[i]
        with zipfile.ZipFile(p["zip_path"]) as z:
            im = Image.open(io.BytesIO(z.read(p["source_image"])))
            want = np.array(im if im.mode in ("RGB", "RGBA") else im.convert("RGB"))
        assert s["source_image"].dtype == torch.uint8 and np.array_equal(s["source_image"].numpy(), want)
    with pytest.raises(MvdError, match="frontend"):
        ObjaverseDataset(frontend="gpu", **kw)
    with pytest.raises(MvdError, match="transform"):
        ObjaverseDataset(frontend="device", transform=lambda x: x, **kw)
    _clear_caches(tree)


def test_retry_pops_pairs_whose_zip_is_gone(tmp_path):
    root = T.build_tree(tmp_path)
    d = ObjaverseDataset(data_root=str(root), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(16, 16), max_views_per_object=2)
    n = len(d)
    gone = d.view_pairs[0]["zip_path"]
    os.remove(gone)
    s = d[0]                                   # the reference's quirk: the pair is popped and index (0 + 1) % len is served
    assert len(d) == n - 1 and s["object_uid"] == d.view_pairs[1]["object_uid"]
    for p in list(d.view_pairs):
        if os.path.exists(p["zip_path"]):
            os.remove(p["zip_path"])
    with pytest.raises(RuntimeError, match="after 3 attempts|Failed to load"):
        d[0]


def test_missing_pillow_is_named(monkeypatch):
    import builtins
    import sys
    from mvd_amd import dataset as D
    from mvd_amd._lib import MvdError
    real = builtins.__import__

    def fake(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", fake)
    for m in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, m)
    with pytest.raises(MvdError, match="Pillow"):
        D._pil()
