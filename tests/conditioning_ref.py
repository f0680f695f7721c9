"""Plain float64 references of the fp32 camera / time conditioning path, one function per operator (mvd_amd/ops.py:
timestep_embedding, camera_features, layernorm_f32, skinny_linear, skinny_linear_grouped, film_params, film_params_grouped,
im2col_in, film_nchw_f32), the full camera embedding, the per-modulator FiLM parameters and the time projection; the bounds
the GPU tests hold the kernels to, and the float32 emulations those bounds are derived from (tests/test_conditioning_ref_cpu.py
runs them).  torch / numpy on the CPU only.  tests/test_conditioning_ref_cpu.py pins the references to oracle/mvd.py and
oracle/sd21_unet.py, which are pinned to the reference project's golden vectors.

Plain helper module (like parity_util.py), no fixtures."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23          # one fp32 ulp of 1.0
LOG_10000 = math.log(10000.0)


def d(t):
    return t.detach().to("cpu", torch.float64)


# ------------------------------------------------------------------------------------------------ sinusoids
def sinusoid_bound(ang, arg):
    """|err| allowed on sin / cos of the float64 angle ``ang = value * exp(arg)`` when value, arg, exp and the product are fp32:
    the angle carries (3 + |arg|) roundings' worth of relative error (the exponent's own, exp's amplification |arg| of it, exp,
    the product, the input), sin / cos turn an angle error into at most the same absolute error, plus one ulp of the result."""
    return ang.abs() * (3.0 + arg.abs()) * EPS32 + EPS32


def timestep_embedding(t, dim):
    """t (B,) -> (emb (B, dim) = [cos | sin], ang (B, dim/2), arg (dim/2,)), float64: diffusers Timesteps(dim, True, 0)"""
    half = dim // 2
    arg = -LOG_10000 * torch.arange(half, dtype=torch.float64) / half
    ang = d(t)[:, None] * torch.exp(arg)[None, :]
    return torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1), ang, arg


def timestep_embedding_bound(ang, arg):
    b = sinusoid_bound(ang, arg[None, :].expand_as(ang))
    return torch.cat([b, b], dim=-1)


def timestep_embedding_f32(t, dim):
    """the kernel's formula step by step in numpy float32: expf(c * i / half), t * f, cosf / sinf"""
    half = dim // 2
    i = np.arange(half, dtype=np.float32)
    f = np.exp(np.float32(-9.210340371976184) * i / np.float32(half)).astype(np.float32)
    ang = (np.asarray(t, dtype=np.float32)[:, None] * f[None, :]).astype(np.float32)
    return torch.from_numpy(np.concatenate([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32))


def relative_transform(src, tgt):
    """cameras (B, 3 or 4, 4) -> R = tR sR^T (B, 3, 3), T = tT - R sT (B, 3), float64 (camera_encoder.py:107-120 of the model)"""
    s, g = d(src), d(tgt)
    sR, sT, tR, tT = s[:, :3, :3], s[:, :3, 3], g[:, :3, :3], g[:, :3, 3]
    R = torch.einsum("bik,bjk->bij", tR, sR)
    T = tT - torch.einsum("bik,bk->bi", R, sT)
    return R, T


def camera_features(src, tgt, nfreq, max_freq=10.0):
    """-> dict(rflat (B, 9), enc (B, 6 nfreq) = per axis [sin nfreq | cos nfreq], ang (B, 3, nfreq), arg (nfreq,),
    rflat_mag (B, 9) = sum of |terms| of every R element), float64"""
    s, g = d(src), d(tgt)
    R, T = relative_transform(src, tgt)
    arg = math.log(max_freq) * torch.arange(nfreq, dtype=torch.float64) / (nfreq - 1)
    ang = T[:, :, None] * torch.exp(arg)[None, None, :]
    enc = torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1).reshape(T.shape[0], -1)
    mag = torch.einsum("bik,bjk->bij", g[:, :3, :3].abs(), s[:, :3, :3].abs())
    return dict(rflat=R.reshape(-1, 9), enc=enc, ang=ang, arg=arg, rflat_mag=mag.reshape(-1, 9), T=T)


def rflat_bound(rflat_mag):
    """4 fp32 ulp of the sum of the magnitudes of an R element's three terms"""
    return 4.0 * ulp32(rflat_mag)


def camera_features_bound(ang, arg):
    b = sinusoid_bound(ang, arg[None, None, :].expand_as(ang))
    return torch.cat([b, b], dim=-1).reshape(ang.shape[0], -1)


def camera_features_f32(src, tgt, nfreq, max_freq=10.0):
    """the kernel's formula step by step in numpy float32 -> (rflat, enc)"""
    s = np.asarray(src, dtype=np.float32)
    g = np.asarray(tgt, dtype=np.float32)
    B = s.shape[0]
    R = np.zeros((B, 3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            a = np.zeros(B, np.float32)
            for k in range(3):
                a = (a + g[:, i, k] * s[:, j, k]).astype(np.float32)
            R[:, i, j] = a
    T = np.zeros((B, 3), np.float32)
    for i in range(3):
        a = g[:, i, 3].copy()
        for k in range(3):
            a = (a - R[:, i, k] * s[:, k, 3]).astype(np.float32)
        T[:, i] = a
    idx = np.arange(nfreq, dtype=np.float32)
    f = np.exp(np.float32(math.log(max_freq)) * idx / np.float32(nfreq - 1)).astype(np.float32)
    ang = (T[:, :, None] * f[None, None, :]).astype(np.float32)
    enc = np.concatenate([np.sin(ang), np.cos(ang)], axis=-1).reshape(B, -1).astype(np.float32)
    return torch.from_numpy(R.reshape(B, 9)), torch.from_numpy(enc)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_f32(x, gamma, beta, eps=1e-5, silu=False, nseg=1):
    """x (rows, c); gamma / beta (c,) or (nseg, c): row r takes the affine of segment r % nseg"""
    x = d(x)
    rows, c = x.shape
    g, b = d(gamma).reshape(nseg, c), d(beta).reshape(nseg, c)
    sel = torch.arange(rows) % nseg
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * g[sel] + b[sel]
    return F.silu(y) if silu else y


def layernorm_f32_emulated(x, gamma, beta, eps=1e-5, silu=False, nseg=1, one_pass=False):
    """The kernel's algorithm in numpy float32: mean, then the sum of squared deviations from it, 1 / sqrt, affine, SiLU as
    t / (1 + exp(-t)).  ``one_pass``: the variance as E[x^2] - mean^2 instead (what the kernel must NOT do)."""
    x = np.asarray(x, dtype=np.float32)
    rows, c = x.shape
    g = np.asarray(gamma, dtype=np.float32).reshape(nseg, c)[np.arange(rows) % nseg]
    b = np.asarray(beta, dtype=np.float32).reshape(nseg, c)[np.arange(rows) % nseg]
    cf = np.float32(c)
    mean = (x.sum(-1, keepdims=True, dtype=np.float32) / cf).astype(np.float32)
    if one_pass:
        var = ((x * x).sum(-1, keepdims=True, dtype=np.float32) / cf - mean * mean).astype(np.float32)
    else:
        dv = (x - mean).astype(np.float32)
        var = ((dv * dv).sum(-1, keepdims=True, dtype=np.float32) / cf).astype(np.float32)
    rstd = (np.float32(1.0) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = ((x - mean) * rstd * g + b).astype(np.float32)
    if silu:
        y = (y / (np.float32(1.0) + np.exp(-y))).astype(np.float32)
    return torch.from_numpy(y)


def layernorm_bound(x, gamma, beta, eps=1e-5, silu=False, nseg=1):
    """4 x the worst error of the two-pass float32 emulation against float64, for this case (a scalar)"""
    want = layernorm_f32(x, gamma, beta, eps, silu, nseg)
    emu = layernorm_f32_emulated(x, gamma, beta, eps, silu, nseg)
    return 4.0 * (emu.double() - want).abs().max().item()


def layernorm_probe(rows=3, c=256, seed=5):
    """rows of mean 100 and standard deviation 0.1: E[x^2] - mean^2 loses every digit of the variance in fp32"""
    g = torch.Generator().manual_seed(seed)
    return (100.0 + 0.1 * torch.randn(rows, c, generator=g)).float()


# ------------------------------------------------------------------------------------------------ linear layers
def linear(x, w, bias=None, silu_in=False):
    x = d(x)
    y = (F.silu(x) if silu_in else x) @ d(w).T
    return y if bias is None else y + d(bias)


def linear_grouped(x, w, seg_end, bias=None, xseg=None):
    """x (B, >= nseg * K): output features [seg_end[g-1], seg_end[g]) read the input columns [g * xseg, g * xseg + K)"""
    x, w = d(x), d(w)
    k = w.shape[1]
    xseg = k if xseg is None else xseg
    outs, o0 = [], 0
    for g, o1 in enumerate(seg_end):
        outs.append(x[:, g * xseg:g * xseg + k] @ w[o0:o1].T)
        o0 = o1
    y = torch.cat(outs, dim=1)
    return y if bias is None else y + d(bias)


def linear_bound(want):
    """the dense skinny_linear test's fp32 figure (tests/test_ops_gpu.py)"""
    return 2e-5 * max(1.0, want.abs().max().item())


# ------------------------------------------------------------------------------------------------ FiLM parameters
def film_params(raw, strength, out_rows=None):
    """raw (B, 2 dim) -> scale = 2 strength sigmoid(raw[:, :dim]), shift = strength raw[:, dim:]; output row r from raw row r % B"""
    raw = d(raw)
    b, dim = raw.shape[0], raw.shape[1] // 2
    sel = torch.arange(b if out_rows is None else out_rows) % b
    return (2.0 * strength * torch.sigmoid(raw[:, :dim]))[sel], (strength * raw[:, dim:])[sel]


def film_params_grouped(raw, seg_end, strength, out_rows=None):
    """-> [(scale, shift)] per segment; ``grouped_layout`` lays them out as the engine does"""
    raw = d(raw)
    res, o0 = [], 0
    for o1 in seg_end:
        res.append(film_params(raw[:, o0:o1], strength, out_rows))
        o0 = o1
    return res


def grouped_layout(pairs):
    """[(scale (rows, dim_g), shift (rows, dim_g))] -> flat: per segment scale | shift (segment g starts at rows * seg_end[g-1])"""
    return torch.cat([t.reshape(-1) for p in pairs for t in p])


def ulp32(v):
    """fp32 ulp of the binade of |v| (float64 tensor), at least the smallest normal's"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 24)


def film_nchw_f32(x, scale, shift):
    """x (B, C, HW), scale / shift (B, C): the float64 fma (the caller rounds it once to fp32)"""
    return d(x) * d(scale)[:, :, None] + d(shift)[:, :, None]


# ------------------------------------------------------------------------------------------------ im2col
def im2col_in(x, scale=None, shift=None, ld_ss=0):
    """x (B, C, H, W) -> (value (B, H, W, 64) float64 BEFORE the bf16 rounding, tap-in-image mask (B, H, W, 64) bool): column
    tap * C + ch of the 3x3 pad-1 window; padding taps and columns 9 C .. 63 are +0 and False.  FiLM: x * scale[b * ld_ss + ch] +
    shift[b * ld_ss + ch] on the taps inside the image only."""
    x = d(x)
    B, C, H, W = x.shape
    if scale is not None:
        sc, sh = d(scale).reshape(-1), d(shift).reshape(-1)
        idx = (torch.arange(B)[:, None] * ld_ss + torch.arange(C)[None, :])
        x = x * sc[idx][:, :, None, None] + sh[idx][:, :, None, None]
    val = torch.zeros(B, H, W, 64, dtype=torch.float64)
    inside = torch.zeros(B, H, W, 64, dtype=torch.bool)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if y0 >= y1 or x0 >= x1:
            continue
        val[:, y0:y1, x0:x1, tap * C:(tap + 1) * C] = x[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx].permute(0, 2, 3, 1)
        inside[:, y0:y1, x0:x1, tap * C:(tap + 1) * C] = True
    return val, inside


def im2col_film_f32(x, scale, shift, ld_ss, fma):
    """the FiLM of im2col_in in fp32 on the CPU, as one fma (one rounding) or as a multiply then an add (two) -> (B, C, H, W)"""
    B, C = x.shape[:2]
    idx = (torch.arange(B)[:, None] * ld_ss + torch.arange(C)[None, :])
    sc, sh = scale.reshape(-1)[idx][:, :, None, None], shift.reshape(-1)[idx][:, :, None, None]
    if fma:
        return (x.double() * sc.double() + sh.double()).float()
    return (x.float() * sc.float()).float() + sh.float()


# ------------------------------------------------------------------------------------------------ camera embedding, FiLM, time
def _ln(x, p, key, silu):
    return layernorm_f32(x, p[f"{key}.weight"], p[f"{key}.bias"], 1e-5, silu)


def _lin(x, p, key):
    return linear(x, p[f"{key}.weight"], p[f"{key}.bias"])


def camera_embedding(p, src, tgt, proj, simple=False):
    """CameraEncoder.encode_cameras in float64 from the per-op references.  p: the encoder's state dict."""
    D = p["output_norm.weight"].shape[0]
    nfreq = (D // 2) // 3
    cf = camera_features(src, tgt, nfreq)

    def mlp(prefix, x):
        x = _ln(_lin(x, p, f"{prefix}.0"), p, f"{prefix}.1", True)
        if simple:
            return _lin(x, p, f"{prefix}.3")
        x = _ln(_lin(x, p, f"{prefix}.3"), p, f"{prefix}.4", True)
        return _lin(x, p, f"{prefix}.6")

    rot = mlp("rotation_encoder", cf["rflat"])
    tr = mlp("translation_encoder", linear(cf["enc"], proj))
    x = torch.cat([rot, tr], dim=-1)
    x = _ln(_lin(x, p, "final_projection.0"), p, "final_projection.1", True)
    x = _ln(_lin(x, p, "final_projection.3"), p, "final_projection.4", False)
    return _ln(x, p, "output_norm", False)


def modulator_film(p, name, emb, strength, out_rows=None):
    """one modulator's (scale, shift) (out_rows, dim) in float64 from an embedding (B, D)"""
    k = f"modulators.{name}"
    x = _ln(_lin(d(emb), p, f"{k}.0"), p, f"{k}.1", True)
    return film_params(_lin(x, p, f"{k}.3"), strength, out_rows)


def bf16_round(t):
    """float64 values rounded once to bf16, back in float64"""
    mant, exp = torch.frexp(d(t))
    return torch.ldexp(torch.round(mant * 256.0) / 256.0, exp)


def resnet_keys(param_names):
    """the resnets in module order, from the parameter names alone: down blocks, the mid block, up blocks, each by index"""
    keys = {n[:-len(".time_emb_proj.weight")] for n in param_names if n.endswith(".time_emb_proj.weight")}
    block = {"down_blocks": 0, "mid_block": 1, "up_blocks": 2}

    def order(k):
        parts = k.split(".")
        return (block[parts[0]],) + tuple(int(s) for s in parts if s.isdigit())
    return sorted(keys, key=order)


def time_projection(p, t, c0):
    """{resnet index: (B, cout)} float64 with the engine's storage precision: bf16 weights (fp32 biases), SiLU(emb) rounded to
    bf16 where the engine stores it; everything else float64.  p: the UNet's state dict, c0 = block_out_channels[0]."""
    emb, _, _ = timestep_embedding(t, c0)
    w = lambda k: d(p[k].to(torch.bfloat16))      # noqa: E731
    h = emb @ w("time_embedding.linear_1.weight").T + d(p["time_embedding.linear_1.bias"])
    h = F.silu(h) @ w("time_embedding.linear_2.weight").T + d(p["time_embedding.linear_2.bias"])
    act = bf16_round(F.silu(h))
    return {i: act @ w(f"{k}.time_emb_proj.weight").T + d(p[f"{k}.time_emb_proj.bias"])
            for i, k in enumerate(resnet_keys(p.keys()))}


def time_projection_f32(p, t, c0):
    """the float32 torch oracle of the same quantity (oracle/sd21_unet.py's own steps, fp32 weights)"""
    from oracle import sd21_unet as OU
    emb = OU.timestep_embedding(t.float(), c0)
    h = F.linear(emb, p["time_embedding.linear_1.weight"], p["time_embedding.linear_1.bias"])
    h = F.silu(F.linear(F.silu(h), p["time_embedding.linear_2.weight"], p["time_embedding.linear_2.bias"]))
    return {i: F.linear(h, p[f"{k}.time_emb_proj.weight"], p[f"{k}.time_emb_proj.bias"])
            for i, k in enumerate(resnet_keys(p.keys()))}


# ------------------------------------------------------------------------------------------------ inputs shared by CPU and GPU tests
def random_cameras(batch, rows=4, seed=0, grid=False):
    """general (NOT orthonormal) random 3x3 blocks and non-zero translations; rows == 4 appends the homogeneous row.
    ``grid``: every entry a non-zero multiple of 1/8 in [-2, 2], so that R and T are exact in fp32 in any order of evaluation --
    the Fourier features' angle then starts from an exact value, like the timestep embedding's, and the sinusoid bound applies to
    it as it stands (with normal entries T cancels to 1 % of its terms in one camera out of a few, and its own fp32 error, not
    the feature formula's, decides the comparison)."""
    g = torch.Generator().manual_seed(1000 + seed)
    if grid:
        draw = lambda: (torch.randint(1, 17, (batch, 3, 4), generator=g) * (torch.randint(0, 2, (batch, 3, 4), generator=g) * 2 - 1)) / 8.0   # noqa: E731
        src, tgt = draw(), draw()
    else:
        src = torch.randn(batch, 3, 4, generator=g)
        tgt = torch.randn(batch, 3, 4, generator=g)
    if rows == 4:
        last = torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(batch, 1, 4)
        src, tgt = torch.cat([src, last], 1), torch.cat([tgt, last], 1)
    return src.contiguous(), tgt.contiguous()


TIMESTEP_DIMS = (2, 32, 258, 320)
TIMESTEP_VALUES = (0.0, 1.0, 500.5, 999.0, -37.25)
CAMERA_NFREQ = (2, 16, 170)
LN_CASES = [(c, rows, silu) for c in (48, 256, 257, 1024) for rows in (1, 5) for silu in (False, True)]


def ln_case(c, rows, silu, nseg=1):
    """x, gamma (nseg, c), beta (nseg, c); every segment's affine differs from every other's at O(0.1)"""
    g = torch.Generator().manual_seed(c * 31 + rows * 7 + int(silu) + 100 * nseg)
    x = (torch.randn(rows, c, generator=g) * 1.5 + 0.3).float()
    gamma = (1.0 + 0.3 * torch.randn(nseg, c, generator=g)).float()
    beta = (0.3 * torch.randn(nseg, c, generator=g)).float()
    return x, gamma, beta


def im2col_film_case(C, h, w, ld_ss, seed=0):
    """inputs of the FiLM im2col cases: x (2, C, h, w), scale, shift (flat, ld_ss + C long at least)"""
    g = torch.Generator().manual_seed(977 * C + 31 * h + w + 7 * ld_ss + seed)
    x = torch.randn(2, C, h, w, generator=g)
    n = max(ld_ss, C) * 2
    scale = (0.4 + 0.2 * torch.rand(n, generator=g)).float()
    shift = (0.3 * torch.randn(n, generator=g)).float()
    return x, scale, shift


def small_cfg():
    """the two-level UNet shape of the small camera engine (tests/test_fixtures_gpu._camera_pair("small"))"""
    from oracle import sd21_unet as OU
    return OU.UNetConfig(block_out_channels=(64, 128), num_heads=(1, 2), cross_attention_dim=64, sample_size=8, layers_per_block=1)


CAM_DIM, CAM_HIDDEN = 96, 48
MAX_CAMERAS = 40


def hooked_modulators(cfg):
    """the modulators the hooks address (``mid`` never is), in the engine's order"""
    from oracle import mvd as OM
    dims = OM.modulation_hidden_dims(cfg)
    n = cfg.num_levels
    return [f"down_{i}" for i in range(n)] + [f"up_{i}" for i in range(n)] + ["output"], dims


def camera_case(which):
    """(encoder state dict, strength, hooked modulator names, {name: dim}, src, tgt, proj) of the camera encoders the row tests run:
    "fixture" -- the bare small engine of tests/test_fixtures_gpu._camera_pair("small"), which lacks two of the hooked modulators
    (embedding tests only: no names); "small" -- the same two-level shape with EVERY hooked modulator, strength 0.5; "tiny" -- the
    tiny model's (parity_util.build_pair, seed 0), strength 0.2.  40 general cameras each; smaller batches are their first rows."""
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    if which == "fixture":
        from tests.test_oracle_golden import _cam_params
        p, strength, names, dims, seed = _cam_params("small"), 0.5, [], {}, 2
    else:
        cfg, seed, strength = (small_cfg(), 3, 0.5) if which == "small" else (OU.UNetConfig.tiny(), 1, 0.2)
        p = OM.init_camera_params(cfg, seed, CAM_DIM, CAM_HIDDEN, False)        # (init_mvd_params(cfg, 0): the encoder takes seed 1)
        names, dims = hooked_modulators(cfg)
    src, tgt = random_cameras(MAX_CAMERAS, 4, seed=50 + seed)
    proj = OM.draw_fourier_projection(CAM_DIM, torch.Generator().manual_seed(60 + seed))
    return p, strength, names, dims, src, tgt, proj


def time_case():
    """(tiny UNet state dict with its 2-D weights rounded to bf16 (what the engine stores), c0, the timestep rows of batch 1, 3, 8)"""
    from oracle import sd21_unet as OU
    cfg = OU.UNetConfig.tiny()
    p = OU.init_params(cfg, 0)
    pb = {k: (v.to(torch.bfloat16).float() if k.endswith(".weight") and v.dim() == 2 else v) for k, v in p.items()}
    vals = (0.0, 321.0, 999.0)
    return pb, cfg.block_out_channels[0], [torch.tensor([vals[(j + b) % 3] for j in range(b)]) for b in (1, 3, 8)]


def time_bound(p, t, c0):
    """({resnet index: (B, cout) bound}, figures) for the time projection, in two stages so that the bf16 store between them is
    treated as what it is.  Stage A, timesteps -> SiLU(emb): the float32 oracle's worst error against float64 in a row is ``worst_a``; an
    activation closer than 8 worst_a to a bf16 rounding tie may be stored one bf16 ulp away from the reference's rounding
    (storage precision, not accumulation order), and is allowed ulp * |W[o][k]| on every output; all others round alike.
    Stage B, the stacked time_emb_proj on identical bf16 activations: 8 x the float32 oracle's worst error ``worst_b``."""
    from oracle import sd21_unet as OU
    keys = resnet_keys(p.keys())
    emb, _, _ = timestep_embedding(t, c0)
    h = emb @ d(p["time_embedding.linear_1.weight"]).T + d(p["time_embedding.linear_1.bias"])
    a64 = F.silu(F.silu(h) @ d(p["time_embedding.linear_2.weight"]).T + d(p["time_embedding.linear_2.bias"]))
    e32 = OU.timestep_embedding(t.float(), c0)
    h32 = F.linear(e32, p["time_embedding.linear_1.weight"], p["time_embedding.linear_1.bias"])
    a32 = F.silu(F.linear(F.silu(h32), p["time_embedding.linear_2.weight"], p["time_embedding.linear_2.bias"]))
    worst_a = (a32.double() - a64).abs().max(dim=1, keepdim=True).values      # per row: t = 0 is exact, t = 999 carries 1e-4 of angle error
    act = bf16_round(a64)
    mant, exp = torch.frexp(a64)
    ulp = torch.ldexp(torch.ones_like(a64), exp - 8)                       # bf16 ulp of the activation's binade
    tie_dist = (((mant.abs() * 256.0) % 1.0) - 0.5).abs() * ulp               # distance of the float64 value from the nearest tie
    near = tie_dist < 8.0 * worst_a
    worst_b, bounds = 0.0, {}
    for i, k in enumerate(keys):
        w, b = p[f"{k}.time_emb_proj.weight"], p[f"{k}.time_emb_proj.bias"]
        want = act @ d(w).T + d(b)
        worst_b = max(worst_b, (F.linear(act.float(), w, b).double() - want).abs().max().item())
    for i, k in enumerate(keys):
        bounds[i] = 8.0 * worst_b + (near.double() * ulp) @ d(p[f"{k}.time_emb_proj.weight"]).abs().T
    return bounds, dict(worst_a=worst_a.max().item(), worst_b=worst_b, near_ties=int(near.sum()), activations=near.numel())


_BOUNDS = {}


def conditioning_bounds():
    """{embedding, film, time} = 8 x {worst_embedding, worst_film, worst_time}, the worst |float32 torch oracle - float64 reference|
    over the row tests' own inputs: the three camera encoders of camera_case at 40 cameras (the smaller batches are their first rows), every hooked
    modulator on the float64 embedding rounded to fp32, and stage B of the tiny model's time projection (time_bound) at batch 1, 3
    and 8."""
    if _BOUNDS:
        return _BOUNDS
    from oracle import mvd as OM
    worst_e = worst_f = 0.0
    for which in ("fixture", "small", "tiny"):
        p, strength, names, _dims, src, tgt, proj = camera_case(which)
        want = camera_embedding(p, src, tgt, proj)
        got = OM.camera_embedding(p, src, tgt, proj)
        worst_e = max(worst_e, (got.double() - want).abs().max().item())
        for name in names:
            sc, sh = modulator_film(p, name, want.float(), strength)
            osc, osh = OM.film_scale_shift(p, name, want.float(), strength)
            worst_f = max(worst_f, (osc.double() - sc).abs().max().item(), (osh.double() - sh).abs().max().item())
    pb, c0, ts = time_case()
    figs = [time_bound(pb, t, c0)[1] for t in ts]
    worst_t = max(f["worst_b"] for f in figs)
    _BOUNDS.update(embedding=8 * worst_e, film=8 * worst_f, time=8 * worst_t, worst_embedding=worst_e, worst_film=worst_f,
                   worst_time=worst_t)
    return _BOUNDS
