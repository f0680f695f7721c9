#!/usr/bin/env python3
"""ms per ``mvd_text_encode`` at SD-2.1 size (OpenCLIP-H text tower: hidden 1024, 23 layers, 16 heads, 77 positions) for
B = 1, 2 (the pipeline's CFG pair), 32, 64: HIP events around each call, warm, median of >= 20 calls, one JSON line per
batch to <out-dir>/text_encoder_b<B>.json.

Next to each time:
* ``weight_bytes``: the bf16 matrices every call streams (23 x (4 H^2 + 2 H I) x 2 bytes = 0.58 GB) and the time those bytes
  take at the HBM bandwidth of MI355X_MICROARCH.md (6.29 TB/s measured float4 copy; 8.0 TB/s spec) -- the batch-1 floor;
* ``flops``: 2 M (4 H^2 + 2 H I) x layers + the attention products, and the achieved rate;
* when ``transformers`` imports: the same ids through ``CLIPTextModel`` in bf16 on the same device (the vendor-stack
  yardstick: hipBLASLt / SDPA through torch), timed the same way.

Weights are seeded random (tests/clip_text_ref.py); time does not depend on their values.  Needs the GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,32,64")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-vendor", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_text_encoder: needs a GPU (a CPU run measures nothing)")
    from mvd_amd.text_encoder import CLIPTextConfigLite, CLIPTextModelHIP
    from tests import clip_text_ref as R
    cfg = R.SD21
    H, I, Lr, T = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["max_position_embeddings"]
    sd = R.seeded_state_dict(cfg, seed=3)
    m = CLIPTextModelHIP(CLIPTextConfigLite(**cfg))
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    vendor = None
    if not a.no_vendor:
        try:
            import transformers
            tc = transformers.CLIPTextConfig(projection_dim=64, pad_token_id=1, bos_token_id=0, eos_token_id=2, **cfg)
            vendor = transformers.CLIPTextModel(tc).eval()
            own = vendor.state_dict()
            pre = "text_model." if any(k.startswith("text_model.") for k in own) else ""
            vendor.load_state_dict({pre + k: v for k, v in sd.items()}, strict=False)
            vendor = vendor.to("cuda", torch.bfloat16)
        except ImportError:
            vendor = None
    os.makedirs(a.out_dir, exist_ok=True)
    wbytes = Lr * (4 * H * H + 2 * H * I) * 2
    for B in (int(b) for b in a.batches.split(",")):
        ids = R.prompt_like_ids(cfg, B, seed=B).cuda()
        M = B * T
        flops = Lr * (2.0 * M * (4 * H * H + 2 * H * I) + 2 * 2.0 * B * (H // 64) * T * T * 64)
        ms = timed(lambda: m(ids), a.warmup, max(a.iters, 20))
        med = statistics.median(ms)
        rec = {"what": "mvd_text_encode, SD-2.1 size (hidden 1024, 23 layers, 16 heads, 77 positions), HIP events, warm",
               "batch": B, "rows": M, "iters": len(ms), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_max": round(max(ms), 4), "weight_bytes": wbytes,
               "floor_ms_hbm_measured_6.29TBs": round(wbytes / HBM_MEASURED * 1e3, 4),
               "floor_ms_hbm_spec_8TBs": round(wbytes / HBM_SPEC * 1e3, 4),
               "weight_stream_TBs": round(wbytes / (med * 1e-3) / 1e12, 3), "flops": flops,
               "tflops": round(flops / (med * 1e-3) / 1e12, 2), "device": torch.cuda.get_device_name(0)}
        if vendor is not None:
            with torch.no_grad():
                vms = timed(lambda: vendor(input_ids=ids)[0], a.warmup, max(a.iters, 20))
            rec["vendor_stack_ms_median"] = round(statistics.median(vms), 4)
            rec["vendor_stack"] = f"transformers {transformers.__version__} CLIPTextModel, bf16, torch {torch.__version__}"
        else:
            rec["vendor_stack_ms_median"] = None
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"text_encoder_b{B}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
