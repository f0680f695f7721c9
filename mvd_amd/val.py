"""The reference's validation script (val.py) on this project's classes: the same metrics, the same two CSV
files with the same columns in the same order and the same aggregation rules, without Lightning, torchmetrics, lpips,
pytorch_msssim, icecream or lovely_tensors.

    python -m mvd_amd.val --ckpt last.ckpt --dataset-path /data/objaverse --config infer_config.yaml --output-dir outputs/val

writes ``<output-dir>/<timestamp>/validation_results.csv`` (one row per sample), ``overall_metrics.csv`` and ``samples/*.png``.

Configuration keys read (the reference ships no ``config/infer_config.yaml``; this is the whole list): ``architecture``,
``torch_dtype``, ``use_camera_conditioning``, ``use_image_conditioning``, ``img_ref_scale``, ``cam_modulation_strength``,
``cam_output_dim``, ``cam_hidden_dim``, ``simple_encoder``, ``scheduler_config`` (optional, ignored as in the reference),
``use_memory_efficient_attention`` / ``enable_gradient_checkpointing`` (optional here, no meaning on this engine), ``image_size``
([width, height]), ``max_views_per_object``, ``batch_size``, ``num_workers``, ``num_inference_steps``, ``guidance_scale``,
``ref_scale``, ``clip_model_name`` (optional); and this project's own optional keys ``cache_dir`` (local huggingface cache of the
architecture and the CLIP snapshot), ``sampler``, ``frontend`` ("host" | "device"), ``extra_metrics``, ``metric_weights`` (a
mapping of the ``ValidationMetrics`` weight keywords to paths), ``group_sources`` and ``guidance_rescale`` (default 0.0: off; the
pipeline's argument of that name, ``--guidance-rescale``) and ``freeu`` (default absent: off; ``"s1,s2,b1,b2"`` or four numbers in
diffusers' ``enable_freeu`` order, ``--freeu``) and ``tome`` (default absent: off; ``"ratio"`` or ``"ratio,max_downsample"``,
``--tome``: token merging, tomesd's ``apply_patch`` names) and ``todo`` (default absent: off; ``"factor"``,
``"factor,factor_level_2"`` or ``"factor,factor_level_2,method"``, ``--todo``: token downsampling of the self-attention keys) and ``deepcache`` (default absent: off; ``"N"`` or ``"N,branch"``, ``--deepcache``) and ``apg`` (default absent: off; ``"eta,norm_threshold,momentum[,space]"``, a
sequence or a mapping, ``--apg``: adaptive projected guidance, the pipeline's argument of that name).

What is kept from the reference on purpose: a metric that cannot be built is ``None`` and scores 0.0; values ``<= 0`` are left out
of the per-metric aggregates; ``clip_score`` is a per-batch value copied to each of the batch's samples and aggregated apart;
PSNR / SSIM / LPIPS / perceptual loss are evaluated again per sample; the comparison image is saved for the LAST sample of each
batch only; a batch that raises is logged and skipped.
"""
from __future__ import annotations

import argparse
import csv
import datetime
import logging
import os
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import MvdError
from .main_options import check_freeu, check_todo, check_tome

logger = logging.getLogger(__name__)

EXTRA_METRICS = ("kid", "is", "prc", "dc")
NOT_AVERAGED = ("clip_score", "batch_inference_time_seconds", "num_samples_in_batch")
DEFAULT_CLIP = "openai/clip-vit-large-patch14"


def _build(what: str, make, level=logging.ERROR):
    try:
        return make()
    except Exception as e:  # noqa: BLE001  (the reference's rule: the run goes on and the metric scores 0.0)
        logger.log(level, "Failed to initialize %s: %s", what, e)
        return None


class ValidationMetrics:
    """The reference's metric set on the N6-N12 classes.  ``*_weights`` / ``*_path`` keywords go to those classes (``None``: their
    own search of the local caches).  ``extra_metrics``: any of "kid", "is", "prc", "dc"; with at least one of them a single
    ``InceptionV3FeaturesHIP`` serves FID and the extras, and every batch costs one tower call per side."""

    def __init__(self, device, clip_model_name: str = DEFAULT_CLIP, *, clip_cache_dir=None, perceptual_weights=None, lpips_backbone=None,
                 lpips_model_path=None, inception_weights=None, extra_metrics: Sequence[str] = (), kid_subsets: int = 100,
                 kid_subset_size: int = 1000, is_splits: int = 10, prc_neighborhood: int = 3, dc_nearest_k: int = 5, max_images_per_pass: int = 8):
        from .clip_score import CLIPScore
        from .fid import FrechetInceptionDistance, InceptionV3FeaturesHIP
        from .lpips import LPIPS
        from .perceptual import PerceptualLoss
        from .validation import SSIM, PeakSignalNoiseRatio
        unknown = [m for m in extra_metrics if m not in EXTRA_METRICS]
        if unknown:
            raise MvdError(f"ValidationMetrics: extra_metrics {unknown}: expected some of {EXTRA_METRICS}")
        self.device = device
        self.extra_metrics = tuple(m for m in EXTRA_METRICS if m in extra_metrics)
        self.ssim = _build("SSIM", lambda: SSIM(data_range=2.0, size_average=True).to(device))
        self.psnr = _build("PSNR", lambda: PeakSignalNoiseRatio(data_range=2.0).to(device))
        self.perceptual_loss = _build("Perceptual loss", lambda: PerceptualLoss(device=device, weights=perceptual_weights))
        self.lpips_metric = _build("LPIPS", lambda: LPIPS(net="alex", backbone=lpips_backbone, model_path=lpips_model_path).to(device))
        self.clip_score_metric = _build("CLIPScore", lambda: CLIPScore(model_name_or_path=clip_model_name, cache_dir=clip_cache_dir).to(device),
                                        logging.WARNING)
        self.inception = None
        if self.extra_metrics:
            self.inception = _build("Inception-v3", lambda: InceptionV3FeaturesHIP(inception_weights, max_images_per_pass=max_images_per_pass),
                                    logging.WARNING)
        shared = dict(inception=self.inception) if self.inception is not None else dict(weights=inception_weights,
                                                                                          max_images_per_pass=max_images_per_pass)
        self.fid_metric = _build("FID", lambda: FrechetInceptionDistance(normalize=True, **shared).to(device), logging.WARNING)
        self.kid_metric = self.is_metric = self.prc_metric = self.dc_metric = None
        if self.inception is not None:
            from .kid import InceptionScore, KernelInceptionDistance
            from .prdc import DensityCoverage, PrecisionRecall
            tower = dict(inception=self.inception, normalize=True)
            if "kid" in self.extra_metrics:
                self.kid_metric = _build("KID", lambda: KernelInceptionDistance(subsets=kid_subsets, subset_size=kid_subset_size, **tower), logging.WARNING)
            if "is" in self.extra_metrics:
                self.is_metric = _build("Inception score", lambda: InceptionScore(splits=is_splits, **tower), logging.WARNING)
            if "prc" in self.extra_metrics:
                self.prc_metric = _build("precision/recall", lambda: PrecisionRecall(neighborhood=prc_neighborhood, **tower), logging.WARNING)
            if "dc" in self.extra_metrics:
                self.dc_metric = _build("density/coverage", lambda: DensityCoverage(nearest_k=dc_nearest_k, **tower), logging.WARNING)

    def _scalar(self, name: str, metric, fn) -> float:
        if metric is None:
            return 0.0
        try:
            return fn()
        except Exception as e:  # noqa: BLE001
            logger.warning("%s calculation failed: %s", name, e)
            return 0.0

    def calculate_metrics(self, generated_images: torch.Tensor, target_images: torch.Tensor, prompts: Optional[List[str]] = None) -> Dict[str, float]:
        """images in [-1, 1]; -> {"psnr", "ssim", "perceptual_loss", "lpips", "clip_score"} of the batch, and the batch is added to
        the FID statistics (and to the extras')"""
        metrics: Dict[str, float] = {}
        with torch.no_grad():
            gen, tgt = generated_images.float(), target_images.float()
            metrics["psnr"] = self._scalar("PSNR", self.psnr, lambda: self.psnr(gen, tgt).item())
            metrics["ssim"] = self._scalar("SSIM", self.ssim, lambda: self.ssim(gen, tgt).item())
            metrics["perceptual_loss"] = self._scalar("Perceptual loss", self.perceptual_loss, lambda: self.perceptual_loss(gen, tgt).item())
            metrics["lpips"] = self._scalar("LPIPS", self.lpips_metric, lambda: self.lpips_metric(gen, tgt).mean().item())

            def clip():
                gen_uint8 = ((gen.clamp(-1, 1) + 1) / 2.0 * 255).to(torch.uint8)
                return self.clip_score_metric(gen_uint8, prompts).item()
            metrics["clip_score"] = self._scalar("CLIP score", self.clip_score_metric if prompts is not None else None, clip)
            if self.fid_metric is not None or self.inception is not None:
                try:
                    gen_fid, tgt_fid = (gen.clamp(-1, 1) + 1) / 2.0, (tgt.clamp(-1, 1) + 1) / 2.0
                    if self.inception is not None:      # the shared tower feeds whichever of FID and the extras were built
                        self._update_shared(self.inception.forward(gen_fid), self.inception.forward(tgt_fid))
                    else:
                        self.fid_metric.update(gen_fid, real=False)
                        self.fid_metric.update(tgt_fid, real=True)
                except Exception as e:  # noqa: BLE001
                    logger.warning("FID update failed: %s", e)
        return metrics

    def _update_shared(self, fake: torch.Tensor, real: torch.Tensor) -> None:
        """one tower call per side feeds every feature metric"""
        for m in (self.fid_metric, self.kid_metric, self.prc_metric, self.dc_metric):
            if m is not None:
                m.update_features(fake, real=False)
                m.update_features(real, real=True)
        if self.is_metric is not None:
            self.is_metric.update_features(fake)

    def compute_fid(self) -> float:
        return self._scalar("FID", self.fid_metric, lambda: self.fid_metric.compute().item())

    def reset_fid(self):
        if self.fid_metric is not None:
            self.fid_metric.reset()

    def compute_extras(self) -> Dict[str, float]:
        """the rows appended to overall_metrics.csv behind the reference's (only for the metrics asked for)"""
        out: Dict[str, float] = {}

        def put(names, metric, what):
            if metric is None:
                vals = [0.0] * len(names)
            else:
                try:
                    vals = [float(v) for v in metric.compute()][:len(names)]
                except Exception as e:  # noqa: BLE001
                    logger.warning("%s computation failed: %s", what, e)
                    vals = [0.0] * len(names)
            out.update(zip(names, vals))
        if "kid" in self.extra_metrics:
            put(("kid_mean", "kid_std"), self.kid_metric, "KID")
        if "is" in self.extra_metrics:
            put(("inception_score_mean", "inception_score_std"), self.is_metric, "Inception score")
        if "prc" in self.extra_metrics:
            put(("precision", "recall", "f_score"), self.prc_metric, "precision/recall")
        if "dc" in self.extra_metrics:
            put(("density", "coverage"), self.dc_metric, "density/coverage")
        return out


# ---------------------------------------------------------------------------------------------------------------- configuration
def load_config(config_path: str) -> Dict:
    if not os.path.exists(config_path):
        raise FileNotFoundError(f"Configuration file not found: {config_path}")
    try:
        import yaml
    except ImportError as e:
        raise MvdError("reading the configuration needs the 'PyYAML' package (yaml), which is not installed") from e
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def setup_pipeline(config: Dict, checkpoint_path: str, device):
    """``create_mvd_pipeline(config["architecture"], ..., text_encoder="hip")`` with the checkpoint's UNet weights, in eval mode on
    ``device``; nothing is fetched (``config["cache_dir"]`` or ``HF_HOME`` names the local cache)"""
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint file not found: {checkpoint_path}")
    from .checkpoint import load_lightning_checkpoint
    from .mvd_unet import create_mvd_pipeline
    pipeline = create_mvd_pipeline(
        pretrained_model_name_or_path=config["architecture"],
        use_memory_efficient_attention=config.get("use_memory_efficient_attention", True),
        enable_gradient_checkpointing=config.get("enable_gradient_checkpointing", False),
        dtype=getattr(torch, config["torch_dtype"]),
        use_camera_conditioning=config["use_camera_conditioning"], use_image_conditioning=config["use_image_conditioning"],
        img_ref_scale=config["img_ref_scale"], cam_modulation_strength=config["cam_modulation_strength"],
        cam_output_dim=config["cam_output_dim"], cam_hidden_dim=config["cam_hidden_dim"], simple_cam_encoder=config["simple_encoder"],
        cache_dir=config.get("cache_dir"), scheduler_config=config.get("scheduler_config", {}), sampler=config.get("sampler", "ddpm"),
        text_encoder="hip")
    missing, unexpected = load_lightning_checkpoint(pipeline.unet, checkpoint_path)
    if missing:
        logger.warning("Missing keys in checkpoint: %s...", missing[:5])
    if unexpected:
        logger.warning("Unexpected keys in checkpoint: %s...", unexpected[:5])
    pipeline = pipeline.to(device)
    for m in (pipeline.unet, pipeline.vae, pipeline.text_encoder):
        if m is not None and hasattr(m, "eval"):
            m.eval()
    return pipeline


# ---------------------------------------------------------------------------------------------------------------- the run
def source_groups(object_uids, prompts, source_camera) -> List[Tuple[int, int]]:
    """``[(first row, end row), ...]`` of a loader batch: consecutive rows that share ``object_uid``, prompt and the bytes of their
    (host) ``source_camera`` are the target views of one source -- one object of a ragged ``generate_views_batch`` call.  The
    dataset emits the pairs of a source one after the other, so with ``max_views_per_object = 4`` a full object gives the spans
    of 3, 2 and 1 rows.  Host work only: nothing here touches the device."""
    cams = [source_camera[i].numpy().tobytes() for i in range(len(object_uids))]
    spans, first = [], 0
    for i in range(1, len(object_uids) + 1):
        if i == len(object_uids) or (object_uids[i], prompts[i], cams[i]) != (object_uids[first], prompts[first], cams[first]):
            spans.append((first, i))
            first = i
    return spans


def run_validation(pipeline, dataset, config: Dict, device, output_dir: Path, *, metrics: Optional[ValidationMetrics] = None,
                   extra_metrics: Sequence[str] = (), metric_kwargs: Optional[Dict] = None, on_batch=None):
    """-> (all_results, overall_metrics) and the two CSV files under ``output_dir``.  ``metrics``: a ready ``ValidationMetrics``
    (otherwise one is built from ``config`` / ``extra_metrics`` / ``metric_kwargs``).  ``on_batch(batch_idx, generated, target,
    prompts)`` (optional) sees every batch's tensors before they are scored.  For a dataset in device mode the loader's workers
    return the raw samples and ``DeviceCollate`` runs here, in the main process (any ``num_workers``).

    ``config["group_sources"]`` (``--group-sources``; default off, and then the run is what it was): the rows of a loader batch that
    share their source (``source_groups``) run as ONE ``generate_views_batch`` call with a ragged camera list -- one encoder pass
    and one copy of the reference K/V per source, every row computed as its own ``batch_size: 1`` call would compute it.  That
    is NOT the default run's result at ``batch_size > 1``, whose ordinary batch couples the rows (Q2 statistics over the batch, Q4
    re-chunking under guidance) and depends on the batch size; rows, columns, CSV order and the timing
    window are the same.  Needs both cameras (a dataset without them runs ungrouped)."""
    from torch.utils.data import DataLoader
    output_dir = Path(output_dir)
    output_dir.mkdir(exist_ok=True, parents=True)
    calc = metrics if metrics is not None else ValidationMetrics(device, config.get("clip_model_name", DEFAULT_CLIP), extra_metrics=extra_metrics,
                                                                 **(metric_kwargs or {}))
    loader_kw = dict(batch_size=config["batch_size"], shuffle=False, num_workers=config["num_workers"])
    device_collate = None
    if getattr(dataset, "frontend", "host") == "device":
        # the workers only inflate and hand the raw arrays back; the copy and the kernels run here, in the process that owns the GPU
        from .dataset import DeviceCollate, raw_collate
        loader_kw["collate_fn"] = raw_collate
        device_collate = DeviceCollate(device, dataset.target_size)
    else:
        loader_kw["pin_memory"] = True
    dataloader = DataLoader(dataset, **loader_kw)
    on_gpu = torch.device(device).type == "cuda"
    all_results, batch_metrics = [], []
    # off (0.0, the default): the pipeline calls are the ones made before the key existed, argument for argument
    rescale = {"guidance_rescale": float(config["guidance_rescale"])} if float(config.get("guidance_rescale", 0.0) or 0.0) != 0.0 else {}
    # FreeU, token merging, token downsampling, DeepCache: absent (the default), the pipeline is not touched
    for key, parse, method in FLAG_OPTIONS:
        setting = parse(config.get(key)) if method else None
        if setting is not None:
            getattr(pipeline, method)(*setting)
    # adaptive projected guidance: absent (the default), the pipeline calls carry no such argument; it rides with the rescale's
    apg = parse_apg(config.get("apg"))
    if apg is not None:
        rescale = dict(rescale, apg=apg)
    with torch.no_grad():
        for batch_idx, batch in enumerate(dataloader):
            try:
                if device_collate is not None:
                    batch = device_collate(batch)
                source_images, target_images = batch["source_image"].to(device), batch["target_image"].to(device)
                source_camera, target_camera = batch.get("source_camera"), batch.get("target_camera")
                prompts, object_uids = batch["prompt"], batch["object_uid"]
                spans = None
                if config.get("group_sources", False) and source_camera is not None and target_camera is not None:
                    spans = source_groups(object_uids, prompts, source_camera.cpu())       # (the loader's cameras are host tensors)
                if source_camera is not None:
                    source_camera = source_camera.to(device)
                if target_camera is not None:
                    target_camera = target_camera.to(device)
                # a host clock around the pipeline call; the device is drained inside the window so that the figure is the work's
                start = time.perf_counter()
                if spans is not None:
                    firsts = [s for s, _ in spans]
                    out = pipeline.generate_views_batch(prompts=[prompts[s] for s in firsts], source_images=source_images[firsts],
                                                        source_cameras=source_camera[firsts], target_cameras=[target_camera[s:e] for s, e in spans],
                                                        num_inference_steps=config["num_inference_steps"], guidance_scale=config["guidance_scale"],
                                                        output_type="pt", **rescale)
                else:
                    out = pipeline(prompt=prompts, num_inference_steps=config["num_inference_steps"], source_camera=source_camera,
                                   target_camera=target_camera, source_images=source_images, guidance_scale=config["guidance_scale"],
                                   ref_scale=config["ref_scale"], output_type="pt", use_camera_embeddings=config["use_camera_conditioning"],
                                   use_image_conditioning=config["use_image_conditioning"], **rescale)
                if on_gpu:
                    torch.cuda.synchronize()
                batch_time = time.perf_counter() - start
                n = len(object_uids)
                logger.info("Batch %d inference time: %.4f seconds for %d samples.", batch_idx, batch_time, n)
                generated_images = (out["images"] * 2.0 - 1.0).to(device)
                if on_batch is not None:
                    on_batch(batch_idx, generated_images, target_images, prompts)
                bm = calc.calculate_metrics(generated_images, target_images, prompts)
                bm["batch_inference_time_seconds"] = batch_time
                bm["num_samples_in_batch"] = n
                per_sample_time = batch_time / n if n > 0 else 0
                again = {"psnr": calc.psnr, "ssim": calc.ssim, "lpips": calc.lpips_metric, "perceptual_loss": calc.perceptual_loss}
                for i in range(n):
                    sample = {"inference_time_seconds": per_sample_time}
                    for name, value in bm.items():
                        if name in NOT_AVERAGED:
                            sample[name] = value              # the batch's value, as it is
                        elif again.get(name) is not None:
                            sample[name] = again[name](generated_images[i:i + 1], target_images[i:i + 1]).item()
                        else:
                            sample[name] = 0.0
                    all_results.append({"object_uid": object_uids[i], "prompt": prompts[i], **sample})
                # (the reference's indentation: behind the loop, so the last sample of the batch)
                save_sample_images(source_images[i], target_images[i], generated_images[i], object_uids[i], sample, output_dir, batch_idx)
                batch_metrics.append(bm)
            except Exception as e:  # noqa: BLE001
                logger.error("Error processing batch %d: %s", batch_idx, e)
                continue
    overall = calculate_overall_metrics(batch_metrics, calc.compute_fid())
    if calc.extra_metrics:
        overall.update(calc.compute_extras())
    save_results(all_results, overall, output_dir)
    return all_results, overall


def save_sample_images(source_image_tensor, target_image_tensor, generated_image_tensor, object_uid, metrics: Dict[str, float], output_dir: Path,
                       batch_idx: int):
    """source | target | generated side by side under a header line, as ``samples/comparison_batch<NNNN>_uid_<uid>.png``"""
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        logger.warning("the 'Pillow' package (PIL) is not installed: no comparison image for UID %s, batch %d", object_uid, batch_idx)
        return
    samples_dir = Path(output_dir) / "samples"
    samples_dir.mkdir(exist_ok=True, parents=True)

    def to_pil(t):
        return Image.fromarray(((t.cpu().permute(1, 2, 0) + 1) / 2 * 255).numpy().astype("uint8"))
    try:
        ims = [to_pil(source_image_tensor), to_pil(target_image_tensor), to_pil(generated_image_tensor)]
        header = 30
        sheet = Image.new("RGB", (sum(im.width for im in ims), ims[0].height + header), (255, 255, 255))
        text = (f"UID: {object_uid} | LPIPS: {metrics.get('lpips', 0.0):.3f} | PSNR: {metrics.get('psnr', 0.0):.2f} | "
                f"SSIM: {metrics.get('ssim', 0.0):.3f}")
        ImageDraw.Draw(sheet).text((10, 5), text, fill="black")
        x = 0
        for im in ims:
            sheet.paste(im, (x, header))
            x += im.width
        sheet.save(samples_dir / f"comparison_batch{batch_idx:04d}_uid_{object_uid}.png")
    except Exception as e:  # noqa: BLE001
        logger.warning("Failed to save sample comparison image for UID %s, batch %d: %s", object_uid, batch_idx, e)


def calculate_overall_metrics(batch_metrics: List[Dict], final_fid: float) -> Dict[str, float]:
    """the reference's aggregation: mean / std / min / max over the batches' values that are > 0 (a metric with none has no rows),
    then ``fid``, then the CLIP score's mean / std over its values > 0, then the timing rows"""
    if not batch_metrics:
        return {}
    agg: Dict[str, float] = {}
    for name in batch_metrics[0].keys():
        if name in NOT_AVERAGED:
            continue
        values = [b[name] for b in batch_metrics if name in b and b[name] > 0]
        if values:
            agg[f"{name}_mean"], agg[f"{name}_std"] = np.mean(values), np.std(values)
            agg[f"{name}_min"], agg[f"{name}_max"] = np.min(values), np.max(values)
    agg["fid"] = final_fid
    clip = [s for s in (b.get("clip_score", 0) for b in batch_metrics) if s > 0]
    if clip:
        agg["clip_score_mean"], agg["clip_score_std"] = np.mean(clip), np.std(clip)
    times = [b["batch_inference_time_seconds"] for b in batch_metrics if "batch_inference_time_seconds" in b]
    counts = [b["num_samples_in_batch"] for b in batch_metrics if "num_samples_in_batch" in b]
    if times:
        agg["mean_batch_inference_time_seconds"], agg["std_batch_inference_time_seconds"] = np.mean(times), np.std(times)
        agg["min_batch_inference_time_seconds"], agg["max_batch_inference_time_seconds"] = np.min(times), np.max(times)
        total, samples = np.sum(times), np.sum(counts)
        agg["total_inference_duration_seconds"] = total
        agg["total_samples_processed_in_inference"] = samples
        agg["avg_per_sample_inference_time_seconds"] = total / samples if samples > 0 else 0.0
    else:
        agg["mean_batch_inference_time_seconds"] = 0.0
        agg["total_inference_duration_seconds"] = 0.0
        agg["total_samples_processed_in_inference"] = 0.0
        agg["avg_per_sample_inference_time_seconds"] = 0.0
    return agg


def save_results(all_results: List[Dict], overall_metrics: Dict, output_dir: Path):
    output_dir = Path(output_dir)
    if all_results:
        with open(output_dir / "validation_results.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=all_results[0].keys())
            w.writeheader()
            w.writerows(all_results)
    with open(output_dir / "overall_metrics.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Metric", "Value"])
        for metric, value in overall_metrics.items():
            w.writerow([metric, value])


def _flag_parts(value, what: str, counts, nums: int = 0):
    """The shared front of the ``parse_*`` below: ``None`` / empty / ``False`` -> ``None`` (off); a string's comma-separated parts, a
    number alone or a sequence's items, the first ``nums`` of them as floats.  ValueError(``what``, got ...) for ``True``, a count
    outside ``counts`` or a part that is no number."""
    if value is None or value == "" or value is False:
        return None
    if isinstance(value, bool):
        raise ValueError(f"{what}, got {value!r}")
    parts = [p.strip() for p in value.split(",")] if isinstance(value, str) else ([value] if isinstance(value, (int, float)) else list(value))
    if len(parts) not in counts:
        raise ValueError(f"{what}, got {value!r}")
    try:
        return [float(p) for p in parts[:nums]] + parts[nums:]
    except (TypeError, ValueError):
        raise ValueError(f"{what}, got {value!r}") from None


def parse_freeu(value):
    """The ``freeu`` config key / ``--freeu`` flag: ``"s1,s2,b1,b2"`` or a sequence of four numbers, in diffusers' ``enable_freeu``
    order -> ``(s1, s2, b1, b2)``; ``None`` / empty -> ``None`` (off).  ValueError for anything else."""
    parts = _flag_parts(value, "freeu: expected four values s1,s2,b1,b2 (SD-2.1: 0.9,0.2,1.4,1.6)", (4,))
    return parts and check_freeu(*parts)


def parse_tome(value):
    """The ``tome`` config key / ``--tome`` flag: ``"ratio"`` or ``"ratio,max_downsample"``, a number, or a sequence of one or two
    numbers, in tomesd's ``apply_patch`` order -> ``(ratio, max_downsample)`` (max_downsample defaults to 1); ``None`` / empty ->
    ``None`` (off).  ValueError for anything else."""
    parts = _flag_parts(value, "tome: expected ratio[,max_downsample] (e.g. 0.5 or 0.5,2)", (1, 2), nums=2)
    if parts is None:
        return None
    ratio, mds = parts[0], parts[1] if len(parts) == 2 else 1.0
    if mds != int(mds):
        raise ValueError(f"tome: max_downsample is one of 1, 2, 4, 8, got {value!r}")
    return check_tome(ratio, int(mds))


def parse_todo(value):
    """The ``todo`` config key / ``--todo`` flag: ``"factor"``, ``"factor,factor_level_2"`` or ``"factor,factor_level_2,method"``, an
    int, or a sequence of one to three such values -> ``(factor, factor_level_2, method)`` (factor_level_2 defaults to 1, the method
    to ``"nearest"``); ``None`` / empty -> ``None`` (off).  ValueError for anything else."""
    parts = _flag_parts(value, "todo: expected factor[,factor_level_2[,method]] (e.g. 2 or 2,1,area)", (1, 2, 3), nums=2)
    if parts is None:
        return None
    fs = parts[:2]
    if any(f != int(f) for f in fs):
        raise ValueError(f"todo: the factors are integers in [1, 4], got {value!r}")
    return check_todo(int(fs[0]), int(fs[1]) if len(fs) == 2 else 1, str(parts[2]) if len(parts) == 3 else "nearest")


def parse_deepcache(value):
    """The ``deepcache`` config key / ``--deepcache`` flag: ``"N"`` or ``"N,branch"``, an int, or a sequence of one or two ints ->
    ``(cache_interval, cache_branch_id)`` (the branch defaults to 0); ``None`` / empty -> ``None`` (off).  ValueError for anything
    else; the branch's upper limit (the UNet's layers_per_block) is checked by ``enable_deepcache``."""
    nums = _flag_parts(value, "deepcache: expected N[,branch] (e.g. 3 or 3,0)", (1, 2), nums=2)
    if nums is None:
        return None
    if any(n != int(n) for n in nums):
        raise ValueError(f"deepcache: the interval and the branch are integers, got {value!r}")
    interval, branch = int(nums[0]), int(nums[1]) if len(nums) == 2 else 0
    if interval < 1 or branch < 0:
        raise ValueError(f"deepcache: the interval must be >= 1 and the branch >= 0, got {value!r}")
    return interval, branch


def parse_apg(value):
    """The ``apg`` config key / ``--apg`` flag: ``"eta,norm_threshold,momentum[,space]"``, a sequence in that order or a mapping of
    those names -> ``mvd_amd.scheduler.APG``; ``None`` / empty -> ``None`` (off).  ValueError for anything else."""
    if value is None or value == "" or value is False:
        return None
    from .scheduler import APG
    if isinstance(value, str) and len(value.split(",")) not in (3, 4):
        raise ValueError(f"apg: expected eta,norm_threshold,momentum[,space] (e.g. 0,15,-0.5), got {value!r}")
    return APG.of(value)


# (config key and flag name, its parser, the pipeline method that takes the parsed value's items; apg rides with the pipeline calls)
FLAG_OPTIONS = (("apg", parse_apg, None), ("freeu", parse_freeu, "enable_freeu"), ("tome", parse_tome, "enable_tome"),
                ("todo", parse_todo, "enable_todo"), ("deepcache", parse_deepcache, "enable_deepcache"))


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    ap = argparse.ArgumentParser(description="Validation of a checkpoint on an Objaverse render tree")
    ap.add_argument("--ckpt", type=str, required=True, help="Path to trained checkpoint")
    ap.add_argument("--dataset-path", type=str, required=True, help="Path to the dataset root (holds renders_final/*.zip)")
    ap.add_argument("--config", type=str, default="config/infer_config.yaml", help="Path to inference configuration file")
    ap.add_argument("--output-dir", type=str, default="outputs/gso_validation", help="Output directory for results")
    ap.add_argument("--extra-metrics", type=str, default=None, help=f"comma-separated subset of {','.join(EXTRA_METRICS)} (default: the config's, else none)")
    ap.add_argument("--frontend", choices=("host", "device"), default=None, help="where composite + resize run (default: the config's, else host)")
    ap.add_argument("--group-sources", action="store_true", default=None,
                    help="run the rows of a batch that share their source as one ragged generate_views_batch call: the batch_size 1 "
                         "result at any batch size (default: the config's group_sources, else off)")
    ap.add_argument("--guidance-rescale", type=float, default=None,
                    help="guidance rescale in [0, 1] (Lin et al. 2024, section 3.4; default: the config's guidance_rescale, else 0.0 = off)")
    ap.add_argument("--freeu", type=str, default=None, metavar="s1,s2,b1,b2",
                    help="FreeU on the UNet's main pass, diffusers' enable_freeu order (SD-2.1: 0.9,0.2,1.4,1.6; default: the config's "
                         "freeu, else off)")
    ap.add_argument("--tome", type=str, default=None, metavar="ratio[,max_downsample]",
                    help="token merging in front of the UNet's self-attention, tomesd's apply_patch names: ratio in [0, 0.75], "
                         "max_downsample one of 1, 2, 4, 8, default 1 (e.g. 0.5; default: the config's tome, else off)")
    ap.add_argument("--todo", type=str, default=None, metavar="factor[,factor_level_2[,method]]",
                    help="token downsampling (ToDo) of the UNet's self-attention keys and values: factors in [1, 4] for the blocks at "
                         "the latent's resolution and one level below (default 1), method nearest (default) or area (e.g. 2 or "
                         "2,1,area; default: the config's todo, else off)")
    ap.add_argument("--deepcache", type=str, default=None, metavar="N[,branch]",
                    help="DeepCache (Ma et al. 2024): the whole UNet at every N-th step, the outermost layers around its stored deep "
                         "feature in between; branch = DeepCache's cache_branch_id, default 0 (e.g. 3 or 3,0; default: the config's "
                         "deepcache, else off)")
    ap.add_argument("--apg", type=str, default=None, metavar="eta,norm_threshold,momentum[,space]",
                    help="adaptive projected guidance (Sadat et al. 2025): eta in [0, 1], norm_threshold >= 0 (0: off), momentum in "
                         "(-1, 1), space output|x0 (e.g. 0,15,-0.5; default: the config's apg, else off)")
    args = ap.parse_args(argv)
    for key, parse, _ in FLAG_OPTIONS:
        if getattr(args, key) is not None:
            try:
                parse(getattr(args, key))
            except ValueError as e:
                ap.error(str(e))
    try:
        config = load_config(args.config)
    except Exception as e:  # noqa: BLE001
        logger.error("Failed to load configuration: %s", e)
        return 1
    if args.group_sources:
        config["group_sources"] = True
    if args.guidance_rescale is not None:
        config["guidance_rescale"] = args.guidance_rescale
    for key, _, _ in FLAG_OPTIONS:
        if getattr(args, key) is not None:
            config[key] = getattr(args, key)
    device =torch.device("cuda" if torch.cuda.is_available() else "cpu")
    output_dir = Path(args.output_dir) / datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
    output_dir.mkdir(exist_ok=True, parents=True)
    extras = args.extra_metrics.split(",") if args.extra_metrics else list(config.get("extra_metrics", ()))
    try:
        pipeline = setup_pipeline(config, args.ckpt, device)
    except Exception as e:  # noqa: BLE001
        logger.error("Failed to setup pipeline: %s", e)
        return 1
    try:
        from .dataset import ObjaverseDataset
        dataset = ObjaverseDataset(data_root=args.dataset_path, split="test", target_size=(config["image_size"][0], config["image_size"][1]),
                                   max_views_per_object=config["max_views_per_object"], frontend=args.frontend or config.get("frontend", "host"))
    except Exception as e:  # noqa: BLE001
        logger.error("Failed to load dataset: %s", e)
        return 1
    try:
        kw = dict(config.get("metric_weights", {}), clip_cache_dir=config.get("cache_dir"))
        all_results, overall = run_validation(pipeline, dataset, config, device, output_dir, extra_metrics=[m for m in extras if m], metric_kwargs=kw)
        logger.info("Calculated metrics: %s", overall)
        logger.info("%d samples scored; results under %s", len(all_results), output_dir)
        return 0
    except Exception as e:  # noqa: BLE001
        logger.error("Validation failed: %s", e)
        return 1


if __name__ == "__main__":
    raise SystemExit(main())
