"""``run_validation`` with ``group_sources`` (N16) on the synthetic Objaverse tree of tests/n13_tree.py, with a stub pipeline and stub
metrics that record what they are given: what is under test is the grouping and the plumbing of ``mvd_amd/val.py``, on the CPU.

* ``--group-sources`` writes the same rows in the same order as the ungrouped run and makes ONE ``generate_views_batch`` call per
  batch, whose per-object camera list is the layout of the batch's sources;
* with ``max_views_per_object = 4`` every full object's layout is (3, 2, 1);
* the group's first source image, prompt and source camera are the object's;
* without the flag the calls are the ones made today (``pipeline(...)`` per batch, no ``generate_views_batch``)."""
import csv

import pytest
import torch

import n13_tree as T
from mvd_amd import val as V

TIMING = ("inference_time_seconds", "batch_inference_time_seconds")


class StubPipeline:
    """every generated image is a function of its row's target camera and source image alone, as an uncoupled model's would be:
    the grouped and the ungrouped run then produce the same rows"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _images(source_images, target_camera):
        level = torch.tanh(target_camera.reshape(target_camera.shape[0], -1).sum(1)).abs().view(-1, 1, 1, 1)
        return (0.5 * source_images.clamp(-1, 1).add(1).div(2) + 0.5 * level).clamp(0, 1)

    def __call__(self, prompt=None, source_camera=None, target_camera=None, source_images=None, **kw):
        self.calls.append(("call", list(prompt), source_images.clone(), source_camera.clone(), target_camera.clone(), kw))
        return {"images": self._images(source_images, target_camera)}

    def generate_views_batch(self, prompts=None, source_images=None, source_cameras=None, target_cameras=None, **kw):
        assert isinstance(target_cameras, list) and len(prompts) == source_images.shape[0] == source_cameras.shape[0] == len(target_cameras)
        self.calls.append(("batch", list(prompts), source_images.clone(), source_cameras.clone(), [t.clone() for t in target_cameras], kw))
        counts = [t.shape[0] for t in target_cameras]
        rows = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
        return {"images": self._images(source_images[rows], torch.cat(target_cameras))}


class StubMetrics:
    extra_metrics = ()

    def __init__(self):
        self.psnr = lambda g, t: ((g - t) ** 2).mean() + 1.0
        self.ssim = lambda g, t: (g * t).mean().abs() + 1.0
        self.lpips_metric = lambda g, t: (g - t).abs().mean() + 1.0
        self.perceptual_loss = lambda g, t: (g - t).abs().max() + 1.0

    def calculate_metrics(self, g, t, prompts):
        return dict(psnr=self.psnr(g, t).item(), ssim=self.ssim(g, t).item(), perceptual_loss=self.perceptual_loss(g, t).item(),
                    lpips=self.lpips_metric(g, t).item(), clip_score=float(len(prompts)))

    def compute_fid(self):
        return 1.0


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    return T.build_tree(tmp_path_factory.mktemp("val_ragged") / "data")


def run(tree, out, batch_size, **cfg):
    from mvd_amd.dataset import ObjaverseDataset
    ds = ObjaverseDataset(data_root=str(tree), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(32, 32), max_views_per_object=4,
                          frontend="host")
    config = dict(batch_size=batch_size, num_workers=0, num_inference_steps=2, guidance_scale=2.0, ref_scale=0.1,
                  use_camera_conditioning=True, use_image_conditioning=True, **cfg)
    pipe = StubPipeline()
    seen = []
    results, overall = V.run_validation(pipe, ds, config, "cpu", out, metrics=StubMetrics(),
                                        on_batch=lambda i, g, t, p: seen.append((i, g.clone(), list(p))))
    return results, overall, pipe.calls, seen, ds


def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("batch_size", [6, 4])
def test_group_sources_writes_the_same_rows_from_one_call_per_batch(tree, tmp_path, batch_size):
    plain = run(tree, tmp_path / "plain", batch_size)
    grouped = run(tree, tmp_path / "grouped", batch_size, group_sources=True)
    n_batches = (len(plain[4]) + batch_size - 1) // batch_size
    assert len(plain[0]) == len(grouped[0]) == len(plain[4]) > 12
    # without the flag: today's calls -- pipeline(...) once per batch with every row's own source, nothing else
    assert [c[0] for c in plain[2]] == ["call"] * n_batches
    assert all(set(c[5]) == {"num_inference_steps", "guidance_scale", "ref_scale", "output_type", "use_camera_embeddings", "use_image_conditioning"}
               for c in plain[2])
    # with it: one generate_views_batch call per batch, and the same rows in the same order (the timing columns aside)
    assert [c[0] for c in grouped[2]] == ["batch"] * n_batches
    assert all(c[5] == dict(num_inference_steps=2, guidance_scale=2.0, output_type="pt") for c in grouped[2])
    for (ia, ga, pa), (ib, gb, pb) in zip(plain[3], grouped[3]):
        assert ia == ib and pa == pb and torch.equal(ga, gb)
    for ra, rb in zip(plain[0], grouped[0]):
        assert list(ra) == list(rb)
        assert {k: v for k, v in ra.items() if k not in TIMING} == {k: v for k, v in rb.items() if k not in TIMING}
    rows_a, rows_b = read_csv(tmp_path / "plain" / "validation_results.csv"), read_csv(tmp_path / "grouped" / "validation_results.csv")
    assert rows_a[0] == rows_b[0] and [r[:2] for r in rows_a] == [r[:2] for r in rows_b]
    assert [r[0] for r in read_csv(tmp_path / "plain" / "overall_metrics.csv")] == [r[0] for r in read_csv(tmp_path / "grouped" / "overall_metrics.csv")]
    # each grouped call against the ungrouped call of the same batch: the spans are the runs of equal (prompt, source camera), the
    # object's source / prompt / source camera are the span's first row's, the target cameras the span's rows
    for (_, prompts, src_img, src_cam, tgt_cam, _), (_, oprompts, osrc_img, osrc_cam, tgt_list, _) in zip(plain[2], grouped[2]):
        counts = [t.shape[0] for t in tgt_list]
        assert sum(counts) == len(prompts) and torch.equal(torch.cat(tgt_list), tgt_cam)
        first = 0
        for o, n in enumerate(counts):
            assert oprompts[o] == prompts[first] and torch.equal(osrc_img[o], src_img[first]) and torch.equal(osrc_cam[o], src_cam[first])
            for r in range(first, first + n):
                assert prompts[r] == prompts[first] and torch.equal(src_cam[r], src_cam[first]) and torch.equal(src_img[r], src_img[first])
            if first + n < len(prompts):            # the next span is another source
                assert not torch.equal(src_cam[first + n], src_cam[first])
            first += n


def test_a_full_objects_layout_is_3_2_1(tree, tmp_path):
    """max_views_per_object = 4: views [a, b, c, d] give the pairs a->b a->c a->d b->c b->d c->d, one after the other -- with a batch
    of six rows per object the layout of every object with four views is (3, 2, 1); an object with three views gives (2, 1)"""
    results, _, calls, _, ds = run(tree, tmp_path, 6, group_sources=True)
    uids = [r["object_uid"] for r in results]
    full = 0
    row = 0
    for _, _, _, _, tgt_list, _ in calls:
        counts = [t.shape[0] for t in tgt_list]
        first = row
        for i, n in enumerate(counts):
            uid = uids[first]
            assert all(u == uid for u in uids[first:first + n])
            if uids.count(uid) == 6 and uids[first:first + 6] == [uid] * 6 and first + 6 <= row + sum(counts) and (first == 0 or uids[first - 1] != uid):
                assert counts[i:i + 3] == [3, 2, 1], counts           # the object's six rows lie in this batch
                full += 1
            first += n
        row += sum(counts)
    assert row == len(uids)
    assert full >= 2, full


def test_source_groups_splits_on_uid_prompt_and_camera_bytes():
    cam = torch.arange(32.0).reshape(2, 4, 4)
    cams = cam[[0, 0, 0, 1, 1, 0]]
    assert V.source_groups(["a"] * 6, ["p"] * 6, cams) == [(0, 3), (3, 5), (5, 6)]
    assert V.source_groups(["a", "a", "b", "b"], ["p"] * 4, cam[[0, 0, 0, 0]]) == [(0, 2), (2, 4)]
    assert V.source_groups(["a"] * 3, ["p", "q", "q"], cam[[0, 0, 0]]) == [(0, 1), (1, 3)]
    near = cam[[0, 0]].clone()
    near[1, 0, 0] = torch.nextafter(near[1, 0, 0], torch.tensor(1.0))            # one bit apart: another source
    assert V.source_groups(["a"] * 2, ["p"] * 2, near) == [(0, 1), (1, 2)]
    assert V.source_groups(["a"], ["p"], cam[:1]) == [(0, 1)]
