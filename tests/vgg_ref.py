"""torchvision's ``vgg16().features[:29]`` and the reference's ``PerceptualLoss`` (src/training/losses.py:21-56) restated with
``F.conv2d`` / ``F.relu`` / ``F.max_pool2d`` only -- torchvision is not installed where this project runs, so this file is what
the GPU tower is compared with; tests/test_perceptual_cpu.py checks it against torchvision's own class where that imports.

The network is pinned by the layer table below (convolutions at 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, a ReLU behind
every one but 28, pools at 4, 9, 16, 23) and its parameter count, 14,714,688 over 26 tensors.

``emulate_bf16`` rounds the normalised input and every post-ReLU map to bf16: the storage points of the GPU path (whose
accumulation is fp32 and whose last convolution writes fp32).  The distance between the emulation and the plain fp32 tower is the
error the number format alone causes; the GPU tests bound the kernels by twice that.

Plain helper module (like clip_vision_ref.py), no fixtures."""
import functools
import math

import torch
import torch.nn.functional as F

CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOLS = (4, 9, 16, 23)
TAPS = {3: "relu1_2", 8: "relu2_2", 15: "relu3_3", 22: "relu4_3"}        # index of the ReLU in front of each pool
PARAMS = 14_714_688
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# the GPU tests' shapes: pairs x H x W (the second has odd pool sizes 7 -> 3 and 5 -> 2; the third runs in passes of 2 + 1)
SHAPES = ((1, 32, 32), (1, 40, 56), (3, 48, 32), (2, 64, 64))


def layer_table():
    """[(index, kind)] of features[:29]: 'conv', 'relu', 'pool'"""
    convs = {i for i, _, _ in CONVS}
    out = []
    for i in range(29):
        out.append((i, "conv" if i in convs else "pool" if i in POOLS else "relu"))
    return out


@functools.lru_cache(maxsize=2)
def synthetic_state_dict(seed=0):
    """He initialisation (std sqrt(2 / (9 cin))) rounded to bf16 -- so packing loses nothing -- and biases 0.05 N(0, 1), under
    torchvision's keys; with them the conv5_3 map has an rms of 1 - 2.7 on ``synthetic_images``."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}
    for idx, cin, cout in CONVS:
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.weight"] = w.to(torch.bfloat16).float()
        sd[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
    return sd


def synthetic_images(batch, h, w, seed=0):
    """smooth structure plus fine noise in [-1, 1]: a bilinear 4x upsample of Gaussian noise + 0.2 N(0, 1), clamped"""
    g = torch.Generator().manual_seed(2000 + seed + 7 * batch + 11 * h + 13 * w)
    low = torch.randn(batch, 3, (h + 3) // 4, (w + 3) // 4, generator=g)
    x = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False) + 0.2 * torch.randn(batch, 3, h, w, generator=g)
    return x.clamp(-1.0, 1.0)


def normalize(x):
    """losses.py:42-46: (x + 1) / 2, then torchvision's Normalize(mean, std)"""
    x = (x + 1) / 2
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def features(sd, x, emulate_bf16=False, taps=False, normalized=False):
    """x (B, 3, H, W) in [-1, 1] (``normalized``: already behind ``normalize``) -> features[:29](normalize(x)), NCHW, in x's
    dtype; ``taps``: (features, {name: post-ReLU map in front of each pool})"""
    dt = x.dtype
    h = x if normalized else normalize(x)
    if emulate_bf16:
        h = _bf(h)
    tapped = {}
    for i, kind in layer_table():
        if kind == "conv":
            h = F.conv2d(h, sd[f"features.{i}.weight"].to(dt), sd[f"features.{i}.bias"].to(dt), padding=1)
        elif kind == "relu":
            h = F.relu(h)
            if emulate_bf16:
                h = _bf(h)
            if i in TAPS:
                tapped[TAPS[i]] = h
        else:
            h = F.max_pool2d(h, 2)
    return (h, tapped) if taps else h


def perceptual_loss(sd, x, y, emulate_bf16=False):
    """PerceptualLoss.__call__: F.mse_loss of the two feature maps"""
    return F.mse_loss(features(sd, x, emulate_bf16), features(sd, y, emulate_bf16))


def rel_l2(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30)).item()


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


@functools.lru_cache(maxsize=8)
def case(pairs, h, w, close=False):
    """One shape's inputs and references, computed once for all the tests that need them (nobody writes to them): images x, y
    (``close``: y = clamp(x + 0.05 N(0, 1))), the fp32 tower's features and taps of the stacked batch [x; y], and the bf16-storage
    emulation's rel-L2 from them per tap (``emu``)."""
    from types import SimpleNamespace
    sd = synthetic_state_dict()
    x = synthetic_images(pairs, h, w, 0)
    if close:
        g = torch.Generator().manual_seed(3000 + pairs + h + w)
        y = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(-1.0, 1.0)
    else:
        y = synthetic_images(pairs, h, w, 1)
    both = torch.cat([x, y])
    with torch.no_grad():
        f, t = features(sd, both, taps=True)
        fe, te = features(sd, both, emulate_bf16=True, taps=True)
    emu = {k: rel_l2(te[k], t[k]) for k in t}
    emu["conv5_3"] = rel_l2(fe, f)
    return SimpleNamespace(sd=sd, x=x, y=y, feat=f, taps=t, emu=emu, feat_emu=fe)
