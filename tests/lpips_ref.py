"""LPIPS v0.1 (``lpips.LPIPS(net="alex" | "vgg")``) restated with ``F.conv2d`` / ``F.relu`` / ``F.max_pool2d`` only -- neither the
``lpips`` package nor torchvision is installed where this project runs, so this file is what the GPU path is compared with;
tests/test_lpips_cpu.py checks it against the package's own class where that imports.

The AlexNet tower is pinned by ``ALEX_LAYERS`` (torchvision's ``alexnet().features[:12]``), the VGG one by vgg_ref.py; the taps are
the ReLU outputs at ``ALEX_TAPS`` and relu1_2, 2_2, 3_3, 4_3, 5_3.  In front: (x - SHIFT) / SCALE.  Per tap
f^ = f / (sqrt(sum_c f^2) + 1e-10), d_l = mean_{h,w} sum_c w_c (f^x - f^y)^2, d = sum_l d_l.

``emulate_bf16`` rounds the scaled input and every post-ReLU map to bf16: the storage points of the GPU path (the fifth VGG tap
stays fp32 there and here).  The distance between the emulation and the plain fp32 tower is the error the number format alone
causes; the GPU tests bound the kernels by twice that.

Plain helper module (like vgg_ref.py), no fixtures."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import vgg_ref as V

# (index, kind, cin, cout, kernel, stride, padding)
ALEX_LAYERS = ((0, "conv", 3, 64, 11, 4, 2), (1, "relu"), (2, "pool"), (3, "conv", 64, 192, 5, 1, 2), (4, "relu"), (5, "pool"),
               (6, "conv", 192, 384, 3, 1, 1), (7, "relu"), (8, "conv", 384, 256, 3, 1, 1), (9, "relu"), (10, "conv", 256, 256, 3, 1, 1),
               (11, "relu"))
ALEX_TAPS = (1, 4, 7, 9, 11)
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
# the GPU tests' shapes, pairs x H x W: the smallest legal size (taps 7^2, 3^2, 1, 1, 1); floors in the stride-4 convolution and
# both pools (taps 11 x 15, 5 x 7, 2 x 3); passes of 2 + 1 pairs; several tiles
SHAPES = {"alex": ((1, 31, 31), (1, 47, 66), (3, 64, 64), (2, 96, 80)), "vgg": V.SHAPES}
CLOSE_SIGMA = 0.05


def alex_tap_sizes(h, w):
    c1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    p1 = ((c1[0] - 3) // 2 + 1, (c1[1] - 3) // 2 + 1)
    p2 = ((p1[0] - 3) // 2 + 1, (p1[1] - 3) // 2 + 1)
    return [c1, p1, p2, p2, p2]


@functools.lru_cache(maxsize=2)
def synthetic_alex_state_dict(seed=0):
    """He initialisation (std sqrt(2 / (k k cin))) rounded to bf16 -- so packing loses nothing -- and biases 0.05 N(0, 1), under
    torchvision's keys"""
    g = torch.Generator().manual_seed(4000 + seed)
    sd = {}
    for layer in ALEX_LAYERS:
        if layer[1] != "conv":
            continue
        idx, _, cin, cout, k, _, _ = layer
        w = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (k * k * cin))
        sd[f"features.{idx}.weight"] = w.to(torch.bfloat16).float()
        sd[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
    return sd


@functools.lru_cache(maxsize=2)
def synthetic_lins(net, seed=0):
    """the linear heads under lpips' keys: |N(0, 1)| / C, shape (1, C, 1, 1)"""
    g = torch.Generator().manual_seed(5000 + seed + (0 if net == "alex" else 1))
    return {f"lin{k}.model.1.weight": (torch.randn(c, generator=g).abs() / c).reshape(1, c, 1, 1) for k, c in enumerate(CHANNELS[net])}


def backbone(net):
    return synthetic_alex_state_dict() if net == "alex" else V.synthetic_state_dict()


def scaling_layer(x):
    shift = torch.tensor(SHIFT, dtype=x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def alex_taps(sd, x, emulate_bf16=False):
    """x (B, 3, H, W) in [-1, 1] -> the five post-ReLU maps of features[:12](scaling_layer(x)), NCHW, in x's dtype"""
    dt = x.dtype
    h = scaling_layer(x)
    if emulate_bf16:
        h = _bf(h)
    taps = []
    for layer in ALEX_LAYERS:
        if layer[1] == "conv":
            idx, _, _, _, _, stride, pad = layer
            h = F.conv2d(h, sd[f"features.{idx}.weight"].to(dt), sd[f"features.{idx}.bias"].to(dt), stride=stride, padding=pad)
        elif layer[1] == "relu":
            h = F.relu(h)
            if emulate_bf16:
                h = _bf(h)
            if layer[0] in ALEX_TAPS:
                taps.append(h)
        else:
            h = F.max_pool2d(h, 3, 2)
    return taps


def vgg_taps(sd, x, emulate_bf16=False):
    """relu1_2, relu2_2, relu3_3, relu4_3 and relu5_3 = relu(features.28) of vgg_ref's tower; its normalisation IS the scaling layer
    (2 mean - 1 = SHIFT, 2 std = SCALE)"""
    feat, t = V.features(sd, x, emulate_bf16=emulate_bf16, taps=True)
    return [t[n] for n in ("relu1_2", "relu2_2", "relu3_3", "relu4_3")] + [F.relu(feat)]


def taps_of(net, sd, x, emulate_bf16=False):
    return alex_taps(sd, x, emulate_bf16) if net == "alex" else vgg_taps(sd, x, emulate_bf16)


def unit(f):
    return f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)


def head(taps_x, taps_y, lins, dtype=torch.float64):
    """the LPIPS head in ``dtype`` on NCHW taps -> (d (B,), per layer (B, 5), [g_l (B, C, h, w)]) with
    g_l = sqrt(w_l) (f^x - f^y), so that d_l = |g_l|^2 / (h w)"""
    per, gs = [], []
    for k, (fx, fy) in enumerate(zip(taps_x, taps_y)):
        w = lins[f"lin{k}.model.1.weight"].to(dtype).reshape(1, -1, 1, 1)
        g = w.sqrt() * (unit(fx.to(dtype)) - unit(fy.to(dtype)))
        gs.append(g)
        per.append(g.pow(2).sum(1).mean((1, 2)))
    per = torch.stack(per, 1)
    return per.sum(1), per, gs


def distance(net, sd, lins, x, y, emulate_bf16=False, dtype=torch.float32):
    """lpips.LPIPS(net)(x, y) restated -> (B,)"""
    n = x.shape[0]
    t = taps_of(net, sd, torch.cat([x, y]).to(dtype), emulate_bf16)
    return head([f[:n] for f in t], [f[n:] for f in t], lins, dtype)[0]


def rel_l2(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30)).item()


def distance_bound(per, eta):
    """|d_gpu - d| of one pair given that its g_l are within eta_l (rel-L2) of the true ones: d_l = |g_l|^2 / hw, so
    |delta d_l| <= d_l (2 eta_l + eta_l^2); per (5,), eta (5,)"""
    return float((per.double() * (2 * eta + eta * eta)).sum())


@functools.lru_cache(maxsize=16)
def case(net, pairs, h, w, close=False):
    """One shape's inputs and references, computed once for all the tests that need them (nobody writes to them): images x, y
    (``close``: y = clamp(x + CLOSE_SIGMA N(0, 1))), the fp32 tower's taps of the stacked batch [x; y], the bf16-storage
    emulation's rel-L2 from them per tap (``emu``), the fp64 head on the fp32 taps (``d`` (pairs,), ``per`` (pairs, 5), ``g``),
    the emulation's rel-L2 on g_l PER PAIR (``eps`` (pairs, 5)), the resulting distance bound per pair with eta = 2 eps
    (``bound``) and the emulation's own distance (``d_emu``)."""
    sd, lins = backbone(net), synthetic_lins(net)
    x = V.synthetic_images(pairs, h, w, 0)
    if close:
        g = torch.Generator().manual_seed(3000 + pairs + h + w)
        y = (x + CLOSE_SIGMA * torch.randn(x.shape, generator=g)).clamp(-1.0, 1.0)
    else:
        y = V.synthetic_images(pairs, h, w, 1)
    both = torch.cat([x, y])
    with torch.no_grad():
        t = taps_of(net, sd, both)
        te = taps_of(net, sd, both, emulate_bf16=True)
        d, per, gs = head([f[:pairs] for f in t], [f[pairs:] for f in t], lins)
        d_emu, _, ge = head([f[:pairs] for f in te], [f[pairs:] for f in te], lins)
    emu = [rel_l2(a, b) for a, b in zip(te, t)]
    eps = torch.tensor([[rel_l2(ge[k][p], gs[k][p]) for k in range(5)] for p in range(pairs)], dtype=torch.float64)
    bound = [distance_bound(per[p], 2 * eps[p]) for p in range(pairs)]
    return SimpleNamespace(net=net, sd=sd, lins=lins, x=x, y=y, taps=t, emu=emu, d=d, per=per, g=gs, eps=eps, bound=bound, d_emu=d_emu)
