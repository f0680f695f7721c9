"""Numpy restatement of the image front end (N13): Pillow's alpha composite on white, its 8-bit two-pass LANCZOS resample and the
loader's normalisation, written from Pillow's behaviour.  The CPU tests pin it to live PIL and to tests/golden/n13_frontend.npz;
the GPU tests compare mvd_op_image_frontend with it.  The keyword switches are the faults the sensitivity test injects."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# (h, w, out_h, out_w) of the issue's cases
CASES = [(64, 64, 32, 32), (53, 47, 32, 32), (20, 24, 32, 32), (32, 64, 32, 32), (64, 32, 32, 32), (32, 32, 32, 32), (7, 5, 32, 32),
         (100, 100, 40, 24), (300, 520, 136, 264)]
KINDS = ("random", "binary", "smooth")


def case_name(case) -> str:
    return "%dx%d_to_%dx%d" % case


def make_input(case, kind: str, channels: int = 4, batch: int = 1) -> np.ndarray:
    """the seeded (batch, h, w, channels) uint8 input of one case: uniform random bytes, random 0 / 255, or a smooth image
    (a smaller batch is a prefix of a larger one)"""
    return _make_input3(case, kind, channels)[:batch]


def _make_input3(case, kind, channels, batch=3):
    h, w = case[0], case[1]
    seed = 1300 + 97 * CASES.index(case) + 7 * KINDS.index(kind) + channels
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, (batch, h, w, channels)).astype(np.uint8)
    if kind == "binary":
        return (rng.randint(0, 2, (batch, h, w, channels)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((batch, h, w, channels), np.uint8)
    for b in range(batch):
        for c in range(channels):
            f, p = rng.uniform(0.02, 0.2, 2), rng.uniform(0, 6.28, 2)
            out[b, :, :, c] = np.round(127.5 + 127.5 * np.sin(f[0] * xx + p[0]) * np.cos(f[1] * yy + p[1])).astype(np.uint8)
    return out


def composite_white(rgba: np.ndarray, general: bool = False) -> np.ndarray:
    """(..., 4) uint8 -> (..., 3) uint8: Image.alpha_composite(opaque white, img).convert("RGB").  general = Pillow's formula with
    its division; otherwise the form the kernel uses (outa255 == 65025 for every pixel, so coef1 = 128 a)."""
    s = rgba[..., :3].astype(np.int64)
    a = rgba[..., 3:4].astype(np.int64)
    if general:
        blend = 255 * (255 - a)
        outa255 = a * 255 + blend
        coef1 = a * 255 * 255 * 128 // outa255
    else:
        coef1 = 128 * a
    coef2 = 255 * 128 - coef1
    tmp = s * coef1 + 255 * coef2 + (0x80 << 7)
    return (((tmp + (tmp >> 8)) >> 8) >> 7).astype(np.uint8)


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x: float, a: float = 3.0) -> float:
    return _sinc(x) * _sinc(x / a) if -a <= x < a else 0.0


def coefficients(n_in: int, n_out: int, support: float = 3.0):
    """one pass: (ksize, bounds [(xmin, count)], kk int32 [out][ksize]) in 2^22 fixed point"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    kk = np.zeros((n_out, ksize), np.int64)
    bounds = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        xmax = min(int(center + sup + 0.5), n_in) - xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            w = lanczos((x + xmin - center + 0.5) / fs, support)
            ws.append(w)
            ww += w
        for x in range(xmax):
            k = ws[x] / ww if ww != 0.0 else ws[x]
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds.append((xmin, xmax))
    return ksize, bounds, kk


def resample_axis(img: np.ndarray, axis: int, n_out: int, support: float = 3.0, rounding: bool = True, clip: bool = True, stats=None):
    """one pass along `axis` of a (..., ) integer array; returns uint8 (clip) or the shifted accumulators (no clip)"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    _, bounds, kk = coefficients(n_in, n_out, support)
    src = np.moveaxis(img.astype(np.int64), axis, -1)
    out = np.empty(src.shape[:-1] + (n_out,), np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        acc = (src[..., xmin:xmin + cnt] * kk[xx, :cnt]).sum(-1) + ((1 << (PRECISION_BITS - 1)) if rounding else 0)
        out[..., xx] = acc >> PRECISION_BITS
    if stats is not None:
        stats.append((int(out.min()), int(out.max())))
    if clip:
        out = np.clip(out, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def resize_u8(rgb: np.ndarray, out_h: int, out_w: int, *, support: float = 3.0, rounding: bool = True, vertical_first: bool = False,
              intermediate_u8: bool = True, stats=None) -> np.ndarray:
    """(B, h, w, 3) uint8 -> (B, out_h, out_w, 3) uint8: horizontal pass, uint8, vertical pass, uint8"""
    order = [(2, out_w), (1, out_h)]
    if vertical_first:
        order.reverse()
    x = rgb
    for i, (axis, n) in enumerate(order):
        last = i == len(order) - 1
        x = resample_axis(x, axis, n, support, rounding, clip=intermediate_u8 or last, stats=stats)
    return np.clip(x, 0, 255).astype(np.uint8)


def normalise(u8: np.ndarray, reciprocal: bool = False) -> np.ndarray:
    """float(byte) / 127.5f - 1.0f in fp32 (reciprocal: the multiply by the rounded reciprocal, a fault)"""
    f = u8.astype(np.float32)
    f = f * np.float32(1.0 / 127.5) if reciprocal else f / np.float32(127.5)
    return f - np.float32(1.0)


def frontend(src: np.ndarray, out_h: int, out_w: int, *, resize_first: bool = False, reciprocal: bool = False, **kw):
    """(B, h, w, 3 | 4) uint8 -> (out_u8 (B, out_h, out_w, 3), out_f32 (B, 3, out_h, out_w))"""
    if src.shape[-1] == 4 and resize_first:       # the fault: resize the four channels, composite afterwards
        planes = [resize_u8(np.repeat(src[..., c:c + 1], 3, -1), out_h, out_w, **kw)[..., :1] for c in range(4)]
        u8 = composite_white(np.concatenate(planes, -1))
    else:
        rgb = composite_white(src) if src.shape[-1] == 4 else src
        u8 = resize_u8(rgb, out_h, out_w, **kw)
    return u8, np.ascontiguousarray(normalise(u8, reciprocal).transpose(0, 3, 1, 2))


def pil_frontend(src: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """the same through live PIL, the reference loader's calls: (B, out_h, out_w, 3) uint8"""
    from PIL import Image
    outs = []
    for img in src:
        im = Image.fromarray(img, "RGBA" if img.shape[-1] == 4 else "RGB")
        if im.mode == "RGBA":
            im = Image.alpha_composite(Image.new("RGBA", im.size, (255, 255, 255, 255)), im)
        im = im.convert("RGB")
        if im.size != (out_w, out_h):
            im = im.resize((out_w, out_h), Image.Resampling.LANCZOS)
        outs.append(np.array(im))
    return np.stack(outs)
