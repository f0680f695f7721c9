"""Records tests/golden/clip_preprocess_cases.npz from Pillow and transformers' ``CLIPImageProcessorPil`` (data only): what the
device preprocessing (mvd_vision_preprocess) and its numpy restatement (tests/clip_vision_ref.py) must reproduce.  Run by
hand where both packages are installed; the tests read the file and need neither.

    python tests/golden/make_clip_image_golden.py

Cases (processor ``size = crop_size = 32``; uint8 inputs ``<name>_in`` (B, 3, H, W), outputs ``<name>_pv`` fp32 (B, 3, 32, 32)):
``r40x56`` (B = 3, distinct images, crop offset in x), ``r56x40`` (offset in y), ``r17x23`` (upsampling), ``r32x32`` (both
passes skipped), ``r64x64``, ``r5x7`` (every tap window clipped at both borders).  ``big_in`` 96 x 64 -> shortest edge 224,
crop 224: ``big_u8`` is the uint8 crop (PIL alone).  ``quant_in`` fp32 (2, 3, 8, 16) in and around [-1, 1] with values on and
next to the quantisation boundaries; ``quant_u8`` = ((x.clamp(-1, 1) + 1) / 2 * 255).to(uint8) by torch on the CPU.
"""
import os

import numpy as np
import torch
from PIL import Image
from transformers import CLIPImageProcessorPil

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_preprocess_cases.npz")
SMALL = {"r40x56": (3, 40, 56), "r56x40": (1, 56, 40), "r17x23": (1, 17, 23), "r32x32": (1, 32, 32), "r64x64": (1, 64, 64), "r5x7": (1, 5, 7)}


def main():
    rng = np.random.default_rng(20240607)
    proc = CLIPImageProcessorPil(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    out = {}
    for name, (b, h, w) in SMALL.items():
        u8 = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
        out[name + "_in"] = u8
        out[name + "_pv"] = proc(images=torch.from_numpy(u8), return_tensors="pt")["pixel_values"].numpy().astype(np.float32)
    big = rng.integers(0, 256, (1, 3, 96, 64), dtype=np.uint8)
    res = np.asarray(Image.fromarray(big[0].transpose(1, 2, 0)).resize((224, 336), Image.BICUBIC)).transpose(2, 0, 1)
    out["big_in"] = big
    out["big_u8"] = np.ascontiguousarray(res[None, :, (336 - 224) // 2:(336 - 224) // 2 + 224, :])
    # quantisation: k / 255 * 2 - 1 lands on the boundary of level k; its fp32 neighbours fall on either side
    levels = np.arange(0, 256, dtype=np.float64)
    edge = (levels / 255 * 2 - 1).astype(np.float32)
    vals = np.concatenate([edge, np.nextafter(edge, np.float32(-2)), np.nextafter(edge, np.float32(2)),
                           np.array([-1.5, -1.0, 1.0, 1.5, 0.0, -0.0, 0.999999, -0.999999], dtype=np.float32)])
    q = np.resize(vals, 3 * 8 * 16 * 2).astype(np.float32).reshape(2, 3, 8, 16)
    out["quant_in"] = q
    out["quant_u8"] = ((torch.from_numpy(q).clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8).numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
