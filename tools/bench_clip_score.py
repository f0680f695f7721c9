#!/usr/bin/env python3
"""CLIP score on the GPU (row N7): preprocess / encode / score of ``mvd_amd.clip_score`` at ViT-L/14 geometry (224 crop, 257
tokens, 24 layers, random weights), B = 1, 8, 32 images of 512 x 512 in [-1, 1].  Warm, HIP events around each call, median of
30 repetitions with min / max; images/s from the median.  One JSON line per batch to <out-dir>/clip_score_b<B>.json.

* ``preprocess``: quantise + both resize passes + crop + normalise -> bf16 patch rows (2 launches);
* ``encode``: patch GEMM ... projection from those rows (``mvd_vision_encode``);
* ``score``: ``image_similarity(a, b)`` = 2 x (preprocess + encode) + the cosine -- what ``compute_losses`` adds per batch.

Where ``transformers`` imports, the same tower as its bf16 ``CLIPVisionModelWithProjection`` on the same device is timed on
ready-made ``pixel_values`` (its PIL preprocessing runs on the host and is not timed), alternating with ``encode`` in one
window; otherwise the record says it was skipped.  Needs the GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L14 = dict(hidden_size=1024, intermediate_size=4096, projection_dim=768, num_hidden_layers=24, num_attention_heads=16, image_size=224,
           patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def timed_alternating(fa, fb, warmup, iters):
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(iters):
        for k, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def stats(ts, images):
    med = statistics.median(ts)
    return {"ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "images_per_s": round(images / med * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-transformers", action="store_true", help="this tower alone (for a run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_clip_score: needs a GPU (a CPU run measures nothing)")
    from mvd_amd.clip_score import clip_cosine
    from mvd_amd.vision_encoder import CLIPImageProcessorLite, CLIPVisionConfigLite, CLIPVisionModelHIP
    torch.manual_seed(0)
    model = CLIPVisionModelHIP(CLIPVisionConfigLite(**L14))
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(0.5)
    model = model.to("cuda")
    proc = CLIPImageProcessorLite()
    hf = None
    if not a.no_transformers:
        try:
            from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
            hf = CLIPVisionModelWithProjection(CLIPVisionConfig(**L14)).to("cuda", torch.bfloat16).eval()
        except ImportError:
            pass
    os.makedirs(a.out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(1)
    for B in (int(b) for b in a.batches.split(",")):
        x = (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
        y = (x + 0.1 * torch.randn(B, 3, a.size, a.size, generator=g).cuda()).clamp(-1, 1).contiguous()
        model._sync()

        def pre():
            model._handle.preprocess(x, True, proc.size, proc.crop_size, proc.image_mean, proc.image_std, True, False)

        def enc():
            return model._encode(None, B)

        def score():
            _, na = model.embed_images(x, proc, quantize=True)
            _, nb = model.embed_images(y, proc, quantize=True)
            return clip_cosine(na, nb)[1]
        pre()
        rec = {"what": f"CLIP score, ViT-L/14 geometry (24 layers, 257 tokens), B = {B} images {a.size} x {a.size}, random weights; warm, HIP events",
               "batch": B, "iters": max(a.iters, 20),
               "preprocess": stats(timed(pre, a.warmup, max(a.iters, 20)), B),
               "encode": stats(timed(enc, a.warmup, max(a.iters, 20)), B),
               "score_two_batches_and_cosine": stats(timed(score, a.warmup, max(a.iters, 20)), 2 * B),
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        val = float(score())
        rec["score_value_finite"] = val == val and abs(val) <= 1 + 1e-5
        if hf is None:
            rec["transformers_bf16"] = "skipped (--no-transformers)" if a.no_transformers else "skipped (transformers does not import here)"
        else:
            pv = torch.randn(B, 3, 224, 224, generator=g).cuda().to(torch.bfloat16)
            with torch.no_grad():       # the two encoders alternating in one timed window
                te, t = timed_alternating(enc, lambda: hf(pixel_values=pv).image_embeds, a.warmup, max(a.iters, 20))
            import transformers
            rec["encode_alternating"] = stats(te, B)
            rec["transformers_bf16"] = dict(stats(t, B), what=f"transformers {transformers.__version__} CLIPVisionModelWithProjection, bf16, eager, "
                                                              "encode only, pixel_values ready on the device, alternating with encode_alternating")
            rec["encode_speedup_over_transformers_bf16_median"] = round(statistics.median(t) / statistics.median(te), 2)
            rec["difference_beyond_spread"] = bool(abs(statistics.median(t) - statistics.median(te)) > max(max(te) - min(te), max(t) - min(t)))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"clip_score_b{B}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
