"""Operator-level wrappers over the C ABI (the same kernels the engine schedules).

Used by the parity tests and for bring-up; tensors are bf16/fp32 CUDA tensors, token-major
(NHWC) activations.  No fallback: everything dispatches into libmvd_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "ops expect contiguous CUDA tensors"
    return C.c_void_p(t.data_ptr())


_s = L.stream


def _bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.dtype == torch.bfloat16, "expected bf16"


def _blocked(w, blocked, k, force_cfg):
    """``blocked=(n, k)``: ``w`` holds packing.block_weight of the [n][k] weight (the small-M kernels' LDS-image layout, read
    with force_cfg + 1000).  Returns (n, force_cfg)."""
    if blocked is None:
        return w.shape[0], force_cfg
    n, kb = blocked
    assert kb == k and w.numel() == n * k and n % 32 == 0 and k % 64 == 0, (tuple(w.shape), blocked, k)
    assert force_cfg >= 100, "the blocked weight layout is read by the small-M kernels only (force_cfg = 100 + 10 * tile + depth)"
    return n, force_cfg + 1000


def linear(a, w, bias=None, a2=None, rowvec=None, rows_per_batch=0, res=None, alpha=1.0, geglu=False,
           out_f32=False, force_cfg=-1, splitk=1, blocked=None):
    """out = alpha*( [a|a2] @ w.T + bias + rowvec[row // rows_per_batch] ) + res.  ``blocked=(n, k)``: ``w`` is
    packing.block_weight of the [n][k] weight (small-M kernels only)."""
    _bf16(a, a2, w, res)
    m, k1 = a.shape
    k2 = a2.shape[1] if a2 is not None else 0
    assert blocked is not None or w.shape[1] == k1 + k2
    n, force_cfg = _blocked(w, blocked, k1 + k2, force_cfg)
    on = n // 2 if geglu else n
    out = torch.empty(m, on, device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    # (+ 4096 words: the tile counters of the small-M kernels' in-kernel split-K combine, MVD_OP_SPLITK_COUNTERS)
    ws = torch.empty(splitk * m * n + 4096, device=a.device, dtype=torch.float32) if splitk > 1 else None
    L.call("mvd_op_linear", _p(a), _p(a2), k1, k2, _p(w), _p(bias), _p(rowvec),
           rowvec.shape[1] if rowvec is not None else 0, rows_per_batch, _p(res), float(alpha), int(geglu),
           _p(out), int(out_f32), m, n, force_cfg, splitk, _p(ws), _s())
    return out


def _pv(t):
    """pointer of a view (None passes): the caller hands over the leading dimension"""
    return None if t is None else C.c_void_p(t.data_ptr())


def linear_ld(a, w, bias=None, a2=None, rowvec=None, rows_per_batch=0, res=None, out=None, alpha=1.0, geglu=False,
              out_f32=False, force_cfg=-1, splitk=1, blocked=None):
    """``linear`` in the forms the engine launches (mvd_op_linear_ld): ``w`` (n, k1 + k2), ``rowvec``, ``res`` and ``out`` may be views
    with ``stride(-1) == 1`` -- row / column slices of wider buffers; the pointers and leading dimensions are read from the views.
    ``out=res`` runs in place; ``out=None`` allocates a dense result.  ``blocked=(n, k, ldw)``: ``w`` is packing.block_weight of
    the (n, k) weight, to be read as if its rows were ``ldw`` apart (the kernels refuse ldw != k: the layout has no row stride)."""
    _bf16(a, a2, w, res)
    m, k1 = a.shape
    k2 = a2.shape[1] if a2 is not None else 0
    ldw = w.stride(0)
    if blocked is not None:
        ldw = blocked[2] if len(blocked) > 2 else k1 + k2
        assert w.is_contiguous()
    else:
        assert w.dim() == 2 and w.shape[1] == k1 + k2 and w.stride(1) == 1, (tuple(w.shape), w.stride())
    n, force_cfg = _blocked(w, None if blocked is None else blocked[:2], k1 + k2, force_cfg)
    on = n // 2 if geglu else n
    if out is None:
        out = torch.empty(m, on, device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.shape == (m, on) and out.stride(1) == 1 and out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    assert res is None or (res.shape == (m, on) and res.stride(1) == 1)
    assert rowvec is None or (rowvec.dtype == torch.float32 and rowvec.dim() == 2 and rowvec.shape[1] == n and rowvec.stride(1) == 1)
    ws = torch.empty(splitk * m * n + 4096, device=a.device, dtype=torch.float32) if splitk > 1 else None
    L.call("mvd_op_linear_ld", _p(a), _p(a2), k1, k2, _pv(w), ldw, _p(bias), _pv(rowvec),
           rowvec.stride(0) if rowvec is not None else 0, rows_per_batch, _pv(res), res.stride(0) if res is not None else 0,
           float(alpha), int(geglu), _pv(out), out.stride(0), int(out_f32), m, n, force_cfg, splitk, _p(ws), _s())
    return out


def ln_linear(x, w_folded, cf, eps=1e-5, geglu=False):
    """LayerNorm(x).W^T + b (optionally GEGLU) in one kernel; (w_folded, cf) from packing.fold_layernorm."""
    _bf16(x, w_folded)
    m, k = x.shape
    n = w_folded.shape[0]
    assert w_folded.shape[1] == k and cf.shape == (2, n) and cf.dtype == torch.float32 and cf.is_contiguous()
    out = torch.empty(m, n // 2 if geglu else n, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_ln_linear", _p(x), k, _p(w_folded), _p(cf[0]), _p(cf[1]), float(eps), int(geglu), _p(out), m, n, _s())
    return out


def linear_xs(x, w_packed, geglu=False, ln=False, eps=1e-5, res=None, csplit=0, k=None):
    """The X-stationary short-K GEMM (gemm_xs.hip): out = LN?(x[:, :k]) @ W.T + b (+ res), or value * gelu(gate).
    ``w_packed`` from packing.pack_xs (bias inside; ``ln``: packed from the fold_layernorm pair)."""
    _bf16(x, w_packed, res)
    m = x.shape[0]
    units, ks1 = w_packed.shape[0], w_packed.shape[1]
    k = (ks1 - 1) * 16 if k is None else k
    n_out = units * 16 if geglu else units * 32
    out = torch.empty(m, n_out, device=x.device, dtype=torch.bfloat16)
    assert x.stride(1) == 1 and (res is None or res.stride(1) == 1)
    L.call("mvd_op_linear_xs", C.c_void_p(x.data_ptr()), x.stride(0), _p(w_packed), m, k, units, int(geglu), int(ln), float(eps),
           C.c_void_p(res.data_ptr()) if res is not None else None, res.stride(0) if res is not None else 0, _p(out), n_out,
           csplit, _s())
    return out


def conv3x3_ws(x, w_packed, bias, n, rowvec=None, res=None, shortcut=None, shortcut2=None, variant=0, upsample=False):
    """The weight-streaming 3x3 convolution of small maps (conv_ws.hip): x (B, H, W, C) bf16 with W in {8, 16, 32}, H * W % 64 == 0,
    B * H * W <= 1024, C % 128 == 0; ``variant`` 0 = the launcher's choice, 1 / 2 force 64- / 128-pixel blocks; ``upsample``: nearest 2x in front of the
    convolution (diffusers' Upsample2D; output 2H x 2W of width 16 or 32, no shortcut); ``w_packed`` from packing.pack_ws (conv weight [n][C][3][3] and, optionally, the 1x1
    shortcut weight over ``shortcut`` | ``shortcut2`` rows); stride 1, padding 1.  Returns (B, H, W, n) bf16."""
    _bf16(x, w_packed, res, shortcut, shortcut2)
    b, h, w, c = x.shape
    out = torch.empty(b, 2 * h if upsample else h, 2 * w if upsample else w, n, device=x.device, dtype=torch.bfloat16)
    assert bias.dtype == torch.float32 and bias.numel() == n and x.is_contiguous()
    assert rowvec is None or (rowvec.dtype == torch.float32 and rowvec.stride(1) == 1)
    pp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    L.call("mvd_op_conv3x3_ws", _p(x), b, h, w, c, _p(w_packed), _p(bias), pp(rowvec), rowvec.stride(0) if rowvec is not None else 0,
           pp(res), pp(shortcut), pp(shortcut2), shortcut.shape[-1] if shortcut is not None else 0,
           shortcut2.shape[-1] if shortcut2 is not None else 0, _p(out), n, int(variant) + (16 if upsample else 0), _s())
    return out


def conv3x3(x, w_packed, bias=None, stride=1, upsample=False, rowvec=None, res=None, shortcut=None,
            shortcut2=None, force_cfg=-1, splitk=1, asym_pad=False, blocked=None):
    """x: (B,H,W,Cin) bf16; w_packed: (Cout, 9*Cin [+ Csc]) bf16 tap-major.  asym_pad (stride 2): zero padding on the
    bottom/right edge only (the VAE's Downsample2D(padding=0)).  ``blocked=(n, k)``: ``w_packed`` is packing.block_weight of
    the [n][k] packed weight (small-M kernels only)."""
    _bf16(x, w_packed, res, shortcut, shortcut2)
    B, H, W, Cin = x.shape
    ktot = 9 * Cin + (shortcut.shape[-1] if shortcut is not None else 0) + (shortcut2.shape[-1] if shortcut2 is not None else 0)
    cout, force_cfg = _blocked(w_packed, blocked, ktot, force_cfg)
    oh = H * 2 if upsample else (H + 1) // 2 if stride == 2 else H
    ow = W * 2 if upsample else (W + 1) // 2 if stride == 2 else W
    out = torch.empty(B, oh, ow, cout, device=x.device, dtype=torch.bfloat16)
    c1 = shortcut.shape[-1] if shortcut is not None else 0
    c2 = shortcut2.shape[-1] if shortcut2 is not None else 0
    ws = torch.empty(splitk * B * oh * ow * cout + 4096, device=x.device, dtype=torch.float32) if splitk > 1 else None
    # (the row vector may be a column slice of a wider fp32 buffer, as the engine's fused time_emb_proj output is)
    assert rowvec is None or (rowvec.is_cuda and rowvec.dtype == torch.float32 and rowvec.dim() == 2 and rowvec.shape[1] == cout
                              and rowvec.stride(1) == 1 and (rowvec.shape[0] == 1 or rowvec.stride(0) >= cout)), \
        "rowvec: (B, cout) fp32 with stride(1) == 1 and stride(0) >= cout"
    L.call("mvd_op_conv3x3", _p(x), B, H, W, Cin, stride, int(upsample), int(asym_pad), _p(w_packed), _p(bias), _pv(rowvec),
           rowvec.stride(0) if rowvec is not None else 0, _p(res), _p(shortcut), _p(shortcut2), c1, c2, _p(out), cout,
           force_cfg, splitk, _p(ws), _s())
    return out


def conv3x3_up4(x, w4, bias=None, force_cfg=-1):
    """conv3x3(upsample=True) as four 2x2 sub-pixel convolutions of the source map (gemm_pp.hip AMODE 4).  x: (B,H,W,Cin) bf16;
    w4: packing.pack_up4 of the fp32 [Cout][Cin][3][3] weight, (4, Cout, 4*Cin) bf16.  Raises for a shape the mode does not take
    (W % 16 != 0 other than W == 8 with even H, Cout % 320, Cin % 64)."""
    _bf16(x, w4)
    B, H, W, Cin = x.shape
    assert w4.dim() == 3 and w4.shape[0] == 4 and w4.shape[2] == 4 * Cin and w4.is_contiguous() and x.is_contiguous(), tuple(w4.shape)
    cout = w4.shape[1]
    out = torch.empty(B, 2 * H, 2 * W, cout, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_conv3x3_up4", _p(x), B, H, W, Cin, _p(w4), _p(bias), _p(out), cout, force_cfg, _s())
    return out


def conv3x3_relu(x, w_packed, bias=None, relu=True, out_f32=False, force_cfg=-1, splitk=1):
    """The VGG tower's convolution (gemm_relu.hip): x (B, H, W, Cin) bf16, w_packed (Cout, 9 * Cin) bf16 in the packed conv
    layout; stride 1, padding 1; out = max(conv + bias, 0) (``relu``) rounded once to bf16, or kept in fp32 (``out_f32``).  The
    lock-step tiles only: force_cfg -1, 3 / 4 / 5 (register staging) or 11 / 12 / 13 (LDS-DMA)."""
    _bf16(x, w_packed)
    B, H, W, Cin = x.shape
    cout = w_packed.shape[0]
    assert w_packed.shape[1] == 9 * Cin, (tuple(w_packed.shape), Cin)
    out = torch.empty(B, H, W, cout, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    ws = torch.empty(splitk * B * H * W * cout, device=x.device, dtype=torch.float32) if splitk > 1 else None
    L.call("mvd_op_conv3x3_relu", _p(x), B, H, W, Cin, _p(w_packed), _p(bias), _p(out), cout, int(relu), int(out_f32), force_cfg,
           splitk, _p(ws), _s())
    return out


def linear_relu(a, w, bias=None, relu=True, out_f32=False, force_cfg=-1, splitk=1):
    """out = max(a @ w.T + bias, 0) on the lock-step tiles (conv1_1 of the VGG tower runs this way over im2col rows)."""
    _bf16(a, w)
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k
    out = torch.empty(m, n, device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    ws = torch.empty(splitk * m * n, device=a.device, dtype=torch.float32) if splitk > 1 else None
    L.call("mvd_op_linear_relu", _p(a), k, _p(w), _p(bias), _p(out), m, n, int(relu), int(out_f32), force_cfg, splitk, _p(ws), _s())
    return out


def maxpool2x2(x, out=None):
    """x (B, H, W, C) bf16, C % 8 == 0 -> (B, H // 2, W // 2, C): 2x2 windows, stride 2, an odd trailing row / column dropped.
    ``out``: a buffer whose first B * (H // 2) * (W // 2) * C elements are written."""
    _bf16(x)
    B, H, W, c = x.shape
    if out is None:
        out = torch.empty(B, H // 2, W // 2, c, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_maxpool2x2", _p(x), B, H, W, c, _p(out), _s())
    return out


def sqdiff_mean(a, b, per_pair=False):
    """a, b (pairs, ...) fp32: (mean of (a - b)^2 over everything as a 0-d device tensor, per-pair means (pairs,) or None); fp64
    sums in a fixed order."""
    _f32_same(a, b)
    pairs = a.shape[0]
    n = a.numel() // pairs
    nbytes = L.check(L.lib().mvd_op_sqdiff_mean_ws_bytes(pairs, n), "mvd_op_sqdiff_mean_ws_bytes")
    ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
    mean = torch.empty((), device=a.device, dtype=torch.float32)
    pp = torch.empty(pairs, device=a.device, dtype=torch.float32) if per_pair else None
    L.call("mvd_op_sqdiff_mean", _p(a), _p(b), pairs, n, _p(mean), _p(pp), _p(ws), nbytes, _s())
    return mean, pp


def im2col_patch(src, scale=None, shift=None, out=None):
    """The im2col rows of the AlexNet front ends (lpips.hip).  ``src`` fp32 (B, 3, H, W): the 11x11 stride-4 pad-2 windows,
    (B * oh * ow, 384) bf16 with oh = (H - 7) // 4 + 1, column (ky * 11 + kx) * 3 + c, columns 363.. zero; ``scale`` / ``shift``
    (three floats each) are applied as x * scale[c] + shift[c] to in-image taps only.  ``src`` bf16 (B, H, W, 64): the 5x5 pad-2
    windows, (B * H * W, 1600), column (ky * 5 + kx) * 64 + c.  ``out``: a buffer whose first rows * columns elements are written."""
    if src.dtype == torch.float32:
        B, c, H, W = src.shape
        assert c == 3
        rows, cols, form = B * ((H - 7) // 4 + 1) * ((W - 7) // 4 + 1), 384, 0
    else:
        _bf16(src)
        B, H, W, c = src.shape
        assert c == 64 and scale is None
        rows, cols, form = B * H * W, 1600, 1
    if out is None:
        out = torch.empty(rows, cols, device=src.device, dtype=torch.bfloat16)
    f3 = lambda v: None if v is None else (C.c_float * 3)(*[float(e) for e in v])      # noqa: E731
    L.call("mvd_op_im2col_patch", _p(src), form, B, H, W, f3(scale), f3(shift), _p(out), _s())
    return out


def maxpool3x3s2(x, out=None):
    """x (B, H, W, C) bf16, C % 8 == 0 -> (B, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C): 3x3 windows, stride 2, no padding.
    ``out``: a buffer whose first output elements are written."""
    _bf16(x)
    B, H, W, c = x.shape
    if out is None:
        out = torch.empty(B, (H - 3) // 2 + 1, (W - 3) // 2 + 1, c, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_maxpool3x3s2", _p(x), B, H, W, c, _p(out), _s())
    return out


def lpips_head(xs, ys, lin_w, relu_in=None, per_layer=False, mean=False):
    """The LPIPS head over up to 8 layers in one launch: see ``mvd_amd.lpips.lpips_head`` -> (per-pair (pairs,) -- ``mean``: their
    mean, 0-d, with no per-pair output -- , per-layer (pairs, layers) or None)."""
    from .lpips import lpips_head as head
    d, dl, _ = head(xs, ys, lin_w, relu_in=relu_in, per_layer=per_layer, mean=mean)
    return d, dl


def conv_relu_slice(x, w_packed, bias, kh, kw, stride=1, pad=(0, 0), cin_off=0, cin=None, out=None, c_off=0, out_f32=False):
    """``mvd_op_conv_relu_slice`` (fid.hip): channels [cin_off, cin_off + cin) of x (B, H, W, ld_in) bf16 -> max(conv + bias, 0) in
    channels [c_off, c_off + cout) of ``out`` (B, oh, ow, ld_out), bf16 or (``out_f32``) fp32; ``out=None``: a buffer of cout
    channels.  w_packed (cout, kh * kw * cin_pad) bf16 (``packing.pack_slice_conv``), bias (cout,) fp32."""
    _bf16(x, w_packed)
    B, H, W, ld_in = x.shape
    cin = ld_in - cin_off if cin is None else cin
    cout = w_packed.shape[0]
    assert w_packed.shape[1] == kh * kw * ((cin + 31) // 32 * 32) and bias.dtype == torch.float32 and bias.numel() == cout
    oh, ow = (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1
    if out is None:
        out = torch.empty(B, oh, ow, cout, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16) and tuple(out.shape[:3]) == (B, oh, ow)
    L.call("mvd_op_conv_relu_slice", _p(x), B, H, W, ld_in, cin_off, cin, _p(w_packed), _p(bias), kh, kw, stride, pad[0], pad[1], cout, _p(out),
           out.shape[3], c_off, int(out_f32), _s())
    return out


POOL3_MODES = {"avg": 0, "max1": 1, "max2": 2}


def pool3x3_slice(x, mode, cin_off=0, c=None, out=None, c_off=0):
    """``mvd_op_pool3x3_slice``: 3x3 pool of channels [cin_off, cin_off + c) of x (B, H, W, ld_in) bf16 into channels [c_off, c_off + c)
    of ``out``.  mode "avg": stride 1, pad 1, the mean over the in-image taps; "max1": stride 1, pad 1; "max2": stride 2, no padding."""
    _bf16(x)
    B, H, W, ld_in = x.shape
    c = ld_in - cin_off if c is None else c
    oh, ow = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == "max2" else (H, W)
    if out is None:
        out = torch.empty(B, oh, ow, c, device=x.device, dtype=torch.bfloat16)
    _bf16(out)
    assert tuple(out.shape[:3]) == (B, oh, ow)
    L.call("mvd_op_pool3x3_slice", _p(x), B, H, W, ld_in, cin_off, c, POOL3_MODES[mode], _p(out), out.shape[3], c_off, _s())
    return out


def resize_tf1(images):
    """``mvd_op_resize_tf1``: (B, 3, H, W) uint8, or fp32 in [0, 1] (quantised as trunc(clamp(x, 0, 1) * 255)) -> (B, 299, 299, 16)
    bf16: the TF1-legacy bilinear resize, (v - 128) / 128, channels 3.. zero."""
    assert images.dtype in (torch.uint8, torch.float32) and images.dim() == 4 and images.shape[1] == 3
    B, _, H, W = images.shape
    out = torch.empty(B, 299, 299, 16, device=images.device, dtype=torch.bfloat16)
    L.call("mvd_op_resize_tf1", _p(images), int(images.dtype == torch.float32), B, H, W, _p(out), _s())
    return out


def global_mean(x):
    """x (B, pixels..., C) fp32 -> (B, C): the sum over the pixels in order, divided by their number"""
    assert x.dtype == torch.float32
    B, c = x.shape[0], x.shape[-1]
    out = torch.empty(B, c, device=x.device, dtype=torch.float32)
    L.call("mvd_op_global_mean", _p(x), B, x.numel() // (B * c), c, _p(out), _s())
    return out


def feature_stats(f, total, cov_sum):
    """``mvd_op_feature_stats``: f (n, d) fp32, d % 64 == 0; in place total (d,) += sum_i f_i, cov_sum (d, d) += sum_i f_i f_i^T, fp64"""
    assert f.dtype == torch.float32 and f.dim() == 2 and total.dtype == torch.float64 and cov_sum.dtype == torch.float64
    n, d = f.shape
    assert total.shape == (d,) and cov_sum.shape == (d, d)
    L.call("mvd_op_feature_stats", _p(f), n, d, _p(total), _p(cov_sum), _s())


def kid_mmd(f_real, f_fake, idx, degree=3, gamma=None, coef=1.0, want_sums=False, ws=None):
    """``mvd_op_kid_mmd``: f_real (n_real, d), f_fake (n_fake, d) fp32, d % 64 == 0; idx (subsets, 2, m) int32, slot 0 rows of
    f_real, slot 1 rows of f_fake (validate them on the host: the kernel only clamps) -> the polynomial-kernel MMD of every
    subset, (subsets,) fp64; with ``want_sums`` also (subsets, 3) fp64 = S_xx, S_yy, S_xy.  ``gamma=None``: 1 / d."""
    assert f_real.dtype == torch.float32 and f_fake.dtype == torch.float32 and f_real.dim() == 2 and f_fake.dim() == 2
    assert idx.dtype == torch.int32 and idx.dim() == 3 and idx.shape[1] == 2
    d = f_real.shape[1]
    assert f_fake.shape[1] == d
    subsets, _, m = idx.shape
    need = L.lib().mvd_op_kid_workspace_bytes(subsets, m)
    if need < 0:
        raise L.MvdError(f"mvd_op_kid_workspace_bytes: {L.last_error()}")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=f_real.device)
    out = torch.empty(subsets, dtype=torch.float64, device=f_real.device)
    sums = torch.empty(subsets, 3, dtype=torch.float64, device=f_real.device) if want_sums else None
    L.call("mvd_op_kid_mmd", _p(f_real), f_real.shape[0], _p(f_fake), f_fake.shape[0], d, _p(idx), subsets, m, int(degree),
           float(1.0 / d if gamma is None else gamma), float(coef), _p(ws), need, _p(sums), _p(out), _s())
    return (out, sums) if want_sums else out


def fc_logits(f, w):
    """``mvd_op_fc_logits``: f (n, d) fp32 . w (classes, d)^T fp32 -> (n, classes) fp32, no bias; a row's logits do not depend on n"""
    assert f.dtype == torch.float32 and w.dtype == torch.float32 and f.dim() == 2 and w.dim() == 2 and f.shape[1] == w.shape[1]
    out = torch.empty(f.shape[0], w.shape[0], dtype=torch.float32, device=f.device)
    L.call("mvd_op_fc_logits", _p(f), f.shape[0], f.shape[1], _p(w), w.shape[0], _p(out), _s())
    return out


def inception_score_chunks(logits, perm, splits):
    """``mvd_op_inception_score``: logits (n, classes) fp32, perm (n,) int32 (row j of the shuffled order is row perm[j]) ->
    exp(mean KL) of every chunk of ``torch.chunk(splits)``, (chunks,) fp64"""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and perm.dtype == torch.int32 and perm.shape == (logits.shape[0],)
    n, classes = logits.shape
    need = L.lib().mvd_op_inception_score_workspace_bytes(n, classes, int(splits))
    if need < 0:
        raise L.MvdError(f"mvd_op_inception_score_workspace_bytes: {L.last_error()}")
    ws = torch.empty(need, dtype=torch.uint8, device=logits.device)
    out = torch.empty(min(int(splits), n), dtype=torch.float64, device=logits.device)
    chunks = C.c_int(0)
    L.call("mvd_op_inception_score", _p(logits), n, classes, _p(perm), int(splits), _p(ws), need, _p(out), C.byref(chunks), _s())
    return out[:chunks.value]


def knn_radii(f, k, force_parts=0, want_list=False, ws=None):
    """``mvd_op_knn_radii``: f (n, d) fp32, d % 64 == 0, 1 <= k <= 15, n >= k + 1 -> radii_sq (n,) fp64, the (k + 1)-th smallest
    squared distance of every row to the rows of f (itself included: ``kthvalue(k + 1)``); with ``want_list`` also the k + 1 smallest
    in ascending order, (n, k + 1).  ``force_parts``: the number of column parts (0: automatic); the bits do not depend on it."""
    assert f.dtype == torch.float32 and f.dim() == 2
    n, d = f.shape
    need = L.lib().mvd_op_knn_radii_workspace_bytes(n, int(k), int(force_parts))
    if need < 0:
        raise L.MvdError(f"mvd_op_knn_radii_workspace_bytes: {L.last_error()}")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=f.device)
    radii = torch.empty(n, dtype=torch.float64, device=f.device)
    knn = torch.empty(n, int(k) + 1, dtype=torch.float64, device=f.device) if want_list else None
    L.call("mvd_op_knn_radii", _p(f), n, d, int(k), int(force_parts), _p(radii), _p(knn), _p(ws), need, _s())
    return (radii, knn) if want_list else radii


def manifold_counts(q, r, radii_sq, closed, want_query=True, want_ref=True):
    """``mvd_op_manifold_counts``: q (nq, d), r (nr, d) fp32, radii_sq (nr,) fp64 -> (hits_per_query (nq,), hits_per_ref (nr,))
    int32: the row and column sums of P[j][i] = D2(q_j, r_i) <= radii_sq[i] (``closed``) or < (not ``closed``); an output that is
    not wanted is None"""
    assert q.dtype == torch.float32 and r.dtype == torch.float32 and q.dim() == 2 and r.dim() == 2 and q.shape[1] == r.shape[1]
    assert radii_sq.dtype == torch.float64 and radii_sq.shape == (r.shape[0],)
    hq = torch.empty(q.shape[0], dtype=torch.int32, device=q.device) if want_query else None
    hr = torch.empty(r.shape[0], dtype=torch.int32, device=q.device) if want_ref else None
    L.call("mvd_op_manifold_counts", _p(q), q.shape[0], _p(r), r.shape[0], q.shape[1], _p(radii_sq), int(bool(closed)), _p(hq), _p(hr), _s())
    return hq, hr


def up4_launches() -> int:
    """Launches of the 2x2 sub-pixel upsampling convolution by this process so far."""
    return int(L.lib().mvd_debug_up4_launches())


def attention(q, k, v, heads, scale=0.125):
    """q: (B,Nq,heads*64) bf16, k/v: (B,Nk,heads*64); row strides may exceed heads*64 (views of fused buffers).
    scale=0 selects the engine's form: q already multiplied by 64^-0.5 * log2(e) (packing.QSCALE)."""
    _bf16(q, k, v)
    B, nq, _ = q.shape
    nk = k.shape[1]
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == nq * q.stride(1) and k.stride(0) == nk * k.stride(1) and v.stride(0) == nk * v.stride(1)
    out = torch.empty(B, nq, heads * 64, device=q.device, dtype=torch.bfloat16)
    L.call("mvd_op_attention", C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), _p(out),
           B, heads, nq, nk, q.stride(1), k.stride(1), v.stride(1), heads * 64, float(scale), _s())
    return out


def attention_grouped(q, k, v, heads, kv_group, scale=0.125):
    """``attention`` with grouped K/V: q (B, Nq, heads*64), k / v (B // kv_group, Nk, heads*64) -- batch element b attends the
    K/V of element b // kv_group (the views of one object share its reference tokens).  kv_group=1 is ``attention``."""
    _bf16(q, k, v)
    B, nq, _ = q.shape
    nk = k.shape[1]
    assert kv_group >= 1 and B % kv_group == 0 and k.shape[0] == B // kv_group and v.shape[0] == B // kv_group, (B, kv_group, k.shape, v.shape)
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == nq * q.stride(1) and k.stride(0) == nk * k.stride(1) and v.stride(0) == nk * v.stride(1)
    out = torch.empty(B, nq, heads * 64, device=q.device, dtype=torch.bfloat16)
    L.call("mvd_op_attention_grouped", C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), _p(out),
           B, heads, nq, nk, q.stride(1), k.stride(1), v.stride(1), heads * 64, float(scale), int(kv_group), _s())
    return out


def attention_objects(q, k, v, heads, kv_group, kv_objects, scale=0.125):
    """``attention_grouped`` for the views of several objects: q (B, Nq, heads*64) with B = g * kv_objects * kv_group rows ordered
    [half j][object o][view]; k / v (kv_objects * g, Nk, heads*64) ordered [object o][half j] -- batch element b attends K/V
    element ``(q % O) * g + q // O`` with ``q = b // kv_group``.  kv_objects=1 is ``attention_grouped``."""
    _bf16(q, k, v)
    B, nq, _ = q.shape
    nk = k.shape[1]
    kvg = max(int(kv_group), 1)
    assert kv_objects >= 0 and B % (kvg * max(int(kv_objects), 1)) == 0 and k.shape[0] == B // kvg and v.shape[0] == B // kvg, (B, kv_group, kv_objects, k.shape, v.shape)
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == nq * q.stride(1) and k.stride(0) == nk * k.stride(1) and v.stride(0) == nk * v.stride(1)
    out = torch.empty(B, nq, heads * 64, device=q.device, dtype=torch.bfloat16)
    L.call("mvd_op_attention_objects", C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), _p(out),
           B, heads, nq, nk, q.stride(1), k.stride(1), v.stride(1), heads * 64, float(scale), int(kv_group), int(kv_objects), _s())
    return out


def attention_mapped(q, k, v, heads, kv_index, scale=0.125):
    """``attention`` with a K/V table: q (B, Nq, heads*64); k / v (kv_elements, Nk, heads*64); batch element b attends K/V element
    ``kv_index[b]`` (a sequence or CPU int tensor of B entries -- ragged view counts per object, any many-to-one map).  The
    library checks every entry on the host (``0 <= kv_index[b] < kv_elements``) before it uploads the table or launches."""
    _bf16(q, k, v)
    B, nq, _ = q.shape
    nk = k.shape[1]
    idx = [int(i) for i in (kv_index.tolist() if isinstance(kv_index, torch.Tensor) else kv_index)]
    if isinstance(kv_index, torch.Tensor):
        assert not kv_index.is_cuda and not kv_index.is_floating_point(), "kv_index: a CPU int tensor"
    assert len(idx) == B and k.shape[0] == v.shape[0], (B, len(idx), k.shape, v.shape)
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == nq * q.stride(1) and k.stride(0) == nk * k.stride(1) and v.stride(0) == nk * v.stride(1)
    out = torch.empty(B, nq, heads * 64, device=q.device, dtype=torch.bfloat16)
    L.call("mvd_op_attention_mapped", C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), _p(out),
           B, heads, nq, nk, q.stride(1), k.stride(1), v.stride(1), heads * 64, float(scale), (C.c_int * B)(*idx), int(k.shape[0]), _s())
    return out


def attention_causal(q, k, v, heads, scale=0.125):
    """The CLIP text encoder's attention: q, k, v (B, n, heads*64) bf16 with n <= 96, key j visible to query i iff j <= i; row
    strides may exceed heads*64 (views of one fused QKV buffer).  scale=0: q already carries 64^-0.5 * log2(e)."""
    _bf16(q, k, v)
    B, n, _ = q.shape
    assert k.shape[1] == n and v.shape[1] == n
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == n * q.stride(1) and k.stride(0) == n * k.stride(1) and v.stride(0) == n * v.stride(1)
    out = torch.empty(B, n, heads * 64, device=q.device, dtype=torch.bfloat16)
    L.call("mvd_op_attention_causal", C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), _p(out),
           B, heads, n, q.stride(1), k.stride(1), v.stride(1), heads * 64, float(scale), _s())
    return out


def attention_split(q, k, v, heads, nsplit):
    """Split-KV attention (engine form: q carries softmax_scale * log2 e); the keys are cut into ``nsplit`` ranges."""
    _bf16(q, k, v)
    B, nq, _ = q.shape
    nk = k.shape[1]
    out = torch.empty(B, nq, heads * 64, device=q.device, dtype=torch.bfloat16)
    ws = torch.empty(int(L.lib().mvd_op_attention_split_ws_bytes(B, heads, nq, nsplit)), device=q.device, dtype=torch.uint8)
    L.call("mvd_op_attention_split", C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), _p(out),
           B, heads, nq, nk, q.stride(1), k.stride(1), v.stride(1), heads * 64, nsplit, _p(ws), _s())
    return out


def _pair_args(p0, p1, heads):
    """ctypes arguments of mvd_debug_attention_pair for two problem dicts (see ``attention_pair``): (ptrs, dims, table0, table1,
    batch, outputs, keep-alive list)"""
    B = p0["q"].shape[0]
    ptrs, dims, tables, outs = [], [], [], []
    for p in (p0, p1):
        q, k, v = p["q"], p["k"], p["v"]
        _bf16(q, k, v)
        nq, nk = q.shape[1], k.shape[1]
        out = p.get("out")
        if out is None:
            out = torch.empty(B, nq, heads * 64, device=q.device, dtype=torch.bfloat16)
        _bf16(out)
        assert q.shape[0] == B and out.shape == (B, nq, heads * 64) and k.shape[0] == v.shape[0] and v.shape[1] == nk, (q.shape, k.shape, v.shape, out.shape)
        for t, n in ((q, nq), (k, nk), (v, nk), (out, nq)):      # (batch strides are n * ld in the hook; one element needs none)
            assert t.is_cuda and t.stride(2) == 1 and (t.shape[0] == 1 or t.stride(0) == n * t.stride(1)), (t.shape, t.stride())
        idx = p.get("kv_index")
        if idx is not None:
            idx = [int(i) for i in (idx.tolist() if isinstance(idx, torch.Tensor) else idx)]
            assert len(idx) == B, (B, len(idx))
        ptrs += [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()]
        dims += [nq, nk, q.stride(1), k.stride(1), v.stride(1), out.stride(1), int(p.get("kv_group", 0)), int(p.get("kv_objects", 0)), int(k.shape[0])]
        tables.append(None if idx is None else (C.c_int * B)(*idx))
        outs.append(out)
    return (C.c_void_p * 8)(*ptrs), (C.c_int * 18)(*dims), tables[0], tables[1], B, outs


def attention_pair_ws(p0, p1, heads, scale=0.125, nsplit=1):
    """the workspace ``attention_pair`` would allocate for these arguments: uint8, or None where the launch is not split"""
    _, dims, t0, t1, B, _ = _pair_args(p0, p1, heads)
    n = int(L.lib().mvd_debug_attention_pair_ws_bytes(dims, t0, t1, B, heads, float(scale), int(nsplit)))
    if n < 0:
        raise L.MvdError(f"mvd_debug_attention_pair_ws_bytes: {L.last_error()}")
    return torch.empty(n, device=p0["q"].device, dtype=torch.uint8) if n else None


def attention_pair(p0, p1, heads, scale=0.125, nsplit=1, ws="own", check=True):
    """Test hook: ONE launch of two attention problems, as the engine issues them for an image-conditioned transformer block.
    ``p0`` / ``p1``: dicts with ``q`` (B, Nq_i, heads*64), ``k`` / ``v`` (E_i, Nk_i, heads*64) -- row strides may exceed heads*64 -- and
    optionally ``out`` (B, Nq_i, heads*64; may be a column range of wider rows), ``kv_group``, ``kv_objects`` (as ``attention_objects``)
    or ``kv_index`` (as ``attention_mapped``).  ``nsplit``: 1 = no split-KV, 2..8 forced, 0 = the engine's own choice.  ``ws``: the
    workspace (``attention_pair_ws``), None for a null pointer; by default one is allocated.  Returns the two outputs;
    ``check=False``: (rc, out0, out1) without raising."""
    ptrs, dims, t0, t1, B, outs = _pair_args(p0, p1, heads)
    if isinstance(ws, str):
        ws = attention_pair_ws(p0, p1, heads, scale, nsplit)
    rc = L.lib().mvd_debug_attention_pair(ptrs, dims, t0, t1, B, heads, float(scale), int(nsplit), _p(ws), _s())
    if not check:
        return rc, outs[0], outs[1]
    if rc != 0:
        raise L.MvdError(f"mvd_debug_attention_pair failed (rc={rc}): {L.last_error()}")
    return outs[0], outs[1]


def groupnorm(x, gamma, beta, groups=32, eps=1e-5, silu=False, x2=None):
    """x: (B,HW,C0) bf16 [, x2: (B,HW,C1) concatenated on channels] -> (B,HW,C0+C1)"""
    _bf16(x, x2)
    B, hw, c0 = x.shape
    c1 = x2.shape[2] if x2 is not None else 0
    y = torch.empty(B, hw, c0 + c1, device=x.device, dtype=torch.bfloat16)
    ws = torch.empty(B * 256 * groups * 2, device=x.device, dtype=torch.float32)   # MVD_GN_MAXCHUNK partial sums
    L.call("mvd_op_groupnorm", _p(x), _p(x2), c0, c1, B, hw, groups, float(eps), _p(gamma), _p(beta), int(silu), _p(y),
           _p(ws), _s())
    return y


def layernorm(x, gamma, beta, eps=1e-5):
    _bf16(x)
    rows, c = x.shape
    y = torch.empty_like(x)
    L.call("mvd_op_layernorm", _p(x), rows, c, float(eps), _p(gamma), _p(beta), _p(y), _s())
    return y


def refnorm(x):
    """(B,HW,C) bf16 -> per-pixel normalisation over (batch, channel) (attention.py:95-103 of the reference)."""
    _bf16(x)
    B, hw, c = x.shape
    y = torch.empty_like(x)
    L.call("mvd_op_refnorm", _p(x), B, hw, c, _p(y), _s())
    return y


def refnorm_grouped(x, group):
    """``refnorm`` with statistics over each run of ``group`` consecutive batch rows: ``group == B`` is ``refnorm``, ``group == 1``
    normalises every row (object) by itself, bit-identical to ``refnorm`` on that row alone."""
    _bf16(x)
    B, hw, c = x.shape
    y = torch.empty_like(x)
    L.call("mvd_op_refnorm_grouped", _p(x), B, int(group), hw, c, _p(y), _s())
    return y


def film(x, scale, shift):
    _bf16(x)
    B, hw, c = x.shape
    y = torch.empty_like(x)
    L.call("mvd_op_film", _p(x), B, hw, c, _p(scale), _p(shift), _p(y), _s())
    return y


def conv_in(x, w, bias):
    """x (B,H,W,Cin) bf16, w (Cout,3,3,Cin) fp32 -> (B,H,W,Cout) bf16"""
    B, H, W, cin = x.shape
    cout = w.shape[0]
    y = torch.empty(B, H, W, cout, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_conv_in", _p(x), B, H, W, cin, _p(w), _p(bias), cout, _p(y), _s())
    return y


def conv_out(x, w, bias):
    """x (B,H,W,C) bf16, w (Cout, 9*C) bf16 -> (B,Cout,H,W) fp32"""
    B, H, W, c = x.shape
    cout = w.shape[0]
    y = torch.empty(B, cout, H, W, device=x.device, dtype=torch.float32)
    L.call("mvd_op_conv_out", _p(x), B, H, W, c, _p(w), _p(bias), cout, _p(y), _s())
    return y


def softmax_rows(s):
    """The VAE attention's row softmax (vae.hip): s (rows, n) fp32 -> (rows, n) bf16 probabilities."""
    assert s.dtype == torch.float32 and s.dim() == 2
    out = torch.empty(s.shape, device=s.device, dtype=torch.bfloat16)
    L.call("mvd_op_softmax_rows", _p(s), s.shape[0], s.shape[1], _p(out), _s())
    return out


def vae_pointwise(x, w, bias):
    """quant_conv / post_quant_conv (vae.hip): x (B, cin, hw) fp32, w (cout, cin), bias (cout,) -> (B, cout, hw); cin, cout <= 8."""
    assert x.dtype == torch.float32 and x.dim() == 3 and w.dtype == torch.float32 and w.shape[1] == x.shape[1] and bias.shape == w.shape[:1]
    B, cin, hw = x.shape
    y = torch.empty(B, w.shape[0], hw, device=x.device, dtype=torch.float32)
    L.call("mvd_op_vae_pointwise", _p(x), B, cin, w.shape[0], hw, _p(w), _p(bias), _p(y), _s())
    return y


# ------------------------------------------------------------------------------------------------ the CLIP towers' own kernels
def _f32(*ts):
    for t in ts:
        if t is not None:
            assert t.dtype == torch.float32, "expected fp32"


def clip_add_ln(x, delta, gamma, beta, eps=1e-5, out_f32=False, tower="text", rows=None, out=None):
    """Residual add + LayerNorm of the CLIP layers (clip_layer.h; ``tower``: the translation unit whose copy runs): x (R, H) fp32
    += delta IN PLACE (delta None: x is not written), -> LN(x) as bf16 or (``out_f32``) fp32.  ``rows`` < R leaves the rows behind
    it alone (tests); ``out``: a caller buffer of the output's type."""
    _f32(x, delta, gamma, beta)
    R, H = x.shape
    rows = R if rows is None else rows
    if out is None:
        out = torch.empty(R, H, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16) and rows <= R and out.numel() >= rows * H
    assert gamma.shape == (H,) and beta.shape == (H,) and (delta is None or delta.numel() >= rows * H)
    L.call(f"mvd_op_{tower}_add_ln", _p(x), _p(delta), _p(gamma), _p(beta), rows, H, float(eps), None if out_f32 else _p(out),
           _p(out) if out_f32 else None, _s())
    return out


def clip_act(x, act, tower="text", n=None, out=None):
    """The CLIP MLP's activation pass: fp32 -> bf16, act 0 gelu (erf), 1 quick_gelu; ``n`` (default: all) elements, n % 8 == 0."""
    _f32(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    n = x.numel() if n is None else n
    assert out.dtype == torch.bfloat16 and n <= x.numel() and n <= out.numel()
    L.call(f"mvd_op_{tower}_act", _p(x), n, int(act), _p(out), _s())
    return out


def text_embed(ids, tok, pos, T, out=None):
    """x[row] = tok[ids[row]] + pos[row % T]: ids (rows,) int32, tok (vocab, H), pos (>= T, H) fp32 -> (rows, H) fp32."""
    _f32(tok, pos)
    assert ids.dtype == torch.int32 and ids.dim() == 1 and pos.shape[0] >= T and pos.shape[1] == tok.shape[1]
    rows, (vocab, H) = ids.shape[0], tok.shape
    if out is None:
        out = torch.empty(rows, H, device=tok.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() >= rows * H
    L.call("mvd_op_text_embed", _p(ids), _p(tok), _p(pos), rows, T, H, vocab, _p(out), _s())
    return out


def vit_patchify(pixel_values, patch_size):
    """(B, 3, S, S) fp32 -> (B * (S / P)^2, roundup(3 P^2, 64)) bf16 patch rows in (c, py, px) order, pad columns zero."""
    _f32(pixel_values)
    B, c, S, S2 = pixel_values.shape
    assert c == 3 and S == S2
    kp = (3 * patch_size ** 2 + 63) // 64 * 64
    out = torch.empty(B * (S // patch_size) ** 2, kp, device=pixel_values.device, dtype=torch.bfloat16)
    L.call("mvd_op_vit_patchify", _p(pixel_values), B, S, patch_size, _p(out), _s())
    return out


def vit_embed_ln(patch_out, cls, pos, gamma, beta, batch, eps=1e-5):
    """[class | patches] + position, then pre_layrnorm: patch_out (batch * (T - 1), H), cls (H,), pos (T, H) -> (batch * T, H) fp32."""
    _f32(patch_out, cls, pos, gamma, beta)
    T, H = pos.shape
    assert patch_out.shape == (batch * (T - 1), H) and cls.shape == (H,) and gamma.shape == (H,) and beta.shape == (H,)
    out = torch.empty(batch * T, H, device=pos.device, dtype=torch.float32)
    L.call("mvd_op_vit_embed_ln", _p(patch_out), _p(cls), _p(pos), _p(gamma), _p(beta), batch, T, H, float(eps), _p(out), _s())
    return out


def vit_fold(x, delta, n=None, out=None):
    """out = x + delta over the first ``n`` (default: all) fp32 elements, n % 4 == 0."""
    _f32(x, delta)
    if out is None:
        out = torch.empty_like(x)
    n = x.numel() if n is None else n
    assert out.dtype == torch.float32 and n <= min(x.numel(), delta.numel(), out.numel())
    L.call("mvd_op_vit_fold", _p(x), _p(delta), n, _p(out), _s())
    return out


def clip_l2norm(x, rows=None):
    """x (R, dim) fp32: the first ``rows`` rows divided by their L2 norm IN PLACE."""
    _f32(x)
    assert x.dim() == 2 and (rows is None or rows <= x.shape[0])
    L.call("mvd_op_clip_l2norm", _p(x), x.shape[0] if rows is None else rows, x.shape[1], _s())
    return x


def clip_linear(a, w, bias=None, out_f32=False, route=None):
    """a (M, K) . w (N, K)^T + bias through the CLIP towers' own GEMM routing (``mvd_debug_clip_linear``) -> (M, N) bf16 / fp32.
    ``route``: a list that receives (small-M tile or -1 for the tiled kernels, split-K factor) of the launch."""
    _bf16(a, w)
    _f32(bias)
    (M, K), N = a.shape, w.shape[0]
    assert w.shape[1] == K
    need = L.lib().mvd_debug_clip_linear_ws_bytes(M, N, K, int(out_f32))
    if need < 0:
        raise L.MvdError(f"mvd_debug_clip_linear_ws_bytes: {L.last_error()}")
    ws = torch.empty(need, device=a.device, dtype=torch.uint8)
    out = torch.empty(M, N, device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    got = (C.c_int * 2)()
    L.call("mvd_debug_clip_linear", _p(a), K, M, _p(w), _p(bias), N, _p(out), int(out_f32), _p(ws), ws.numel(), got, _s())
    if route is not None:
        route.append((got[0], got[1]))
    return out


def clip_attention(qkv, batch, heads):
    """The image tower's attention launch (``mvd_debug_clip_attention``): qkv (batch * T, 3 * heads * 64) bf16, q prescaled -> (batch * T, heads * 64)."""
    _bf16(qkv)
    M, w = qkv.shape
    assert w == 3 * heads * 64 and M % batch == 0
    out = torch.empty(M, heads * 64, device=qkv.device, dtype=torch.bfloat16)
    L.call("mvd_debug_clip_attention", _p(qkv), _p(out), batch, heads, M // batch, _s())
    return out


def ddpm_step(model_out, sample, noise, c0, c1, c2, c3, sigma):
    """fp32: x0 = c0*model_out + c1*sample ; prev = c2*x0 + c3*sample + sigma*noise (noise may be None iff sigma == 0)."""
    assert model_out.dtype == torch.float32 and sample.dtype == torch.float32
    out = torch.empty_like(sample)
    L.call("mvd_op_ddpm_step", _p(model_out), _p(sample), _p(noise), float(c0), float(c1), float(c2), float(c3),
           float(sigma), _p(out), sample.numel(), _s())
    return out


def cfg_combine(uncond_cond, guidance_scale):
    """(2B, ...) fp32 [uncond | cond] -> (B, ...) uncond + g*(cond - uncond)."""
    assert uncond_cond.dtype == torch.float32 and uncond_cond.shape[0] % 2 == 0
    out = torch.empty((uncond_cond.shape[0] // 2,) + tuple(uncond_cond.shape[1:]), device=uncond_cond.device,
                      dtype=torch.float32)
    L.call("mvd_op_cfg_combine", _p(uncond_cond), float(guidance_scale), _p(out), out.numel(), _s())
    return out


def sampler_step(model_out, sample, a0, a1, p, q, r=0.0, sigma=0.0, x0_prev=None, noise=None, guidance_scale=None,
                 out=None, x0_out=None):
    """fp32 DDIM / DPM-Solver++ step: m = model_out, or u + g*(c - u) of the stacked (2B, ...) [uncond | cond] when
    ``guidance_scale`` is given; x0 = a0*m + a1*sample ; out = p*sample + q*x0 + r*x0_prev + sigma*noise ; x0_out = x0.
    ``x0_prev`` may be None iff r == 0, ``noise`` iff sigma == 0.  ``out`` may be ``sample`` and ``x0_out`` may be ``x0_prev``."""
    guided = guidance_scale is not None
    assert model_out.dtype == torch.float32 and sample.dtype == torch.float32
    assert model_out.numel() == sample.numel() * (2 if guided else 1), (tuple(model_out.shape), tuple(sample.shape))
    for t in (x0_prev, noise, out, x0_out):
        assert t is None or (t.dtype == torch.float32 and t.numel() == sample.numel())
    if out is None:
        out = torch.empty_like(sample)
    L.call("mvd_op_sampler_step", _p(model_out), int(guided), float(guidance_scale) if guided else 0.0, _p(sample), _p(x0_prev),
           _p(noise), float(a0), float(a1), float(p), float(q), float(r), float(sigma), _p(out), _p(x0_out), sample.numel(), _s())
    return out


def _rescale_rows(uncond_cond):
    """(rows, n_row) of a stacked (2 * rows, ...) [uncond | cond] model output: guidance rescale works per batch row."""
    if uncond_cond.dim() < 2 or uncond_cond.shape[0] % 2:
        raise L.MvdError(f"guidance rescale: expected [uncond | cond] of shape (2 * rows, ...), got {tuple(uncond_cond.shape)}")
    if not (uncond_cond.is_cuda and uncond_cond.dtype == torch.float32 and uncond_cond.is_contiguous()):
        raise L.MvdError(f"guidance rescale: expected a contiguous fp32 CUDA tensor, got {uncond_cond.dtype} on {uncond_cond.device}")
    rows = uncond_cond.shape[0] // 2
    return rows, uncond_cond.numel() // (2 * rows)


def cfg_rescale(uncond_cond, guidance_scale, guidance_rescale, out=None):
    """(2B, ...) fp32 [uncond | cond] -> (B, ...): the guided output m = u + g*(c - u) with guidance rescale (Lin et al. 2024, 3.4;
    diffusers' ``rescale_noise_cfg``): per batch row, m * (phi * std(c) / std(m) + 1 - phi), unbiased std over the row, no
    epsilon.  One launch (``mvd_op_cfg_rescale``).  ``out`` must not overlap ``uncond_cond``."""
    rows, n_row = _rescale_rows(uncond_cond)
    if out is None:
        out = torch.empty((rows,) + tuple(uncond_cond.shape[1:]), device=uncond_cond.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() == rows * n_row and out.is_contiguous()
    L.call("mvd_op_cfg_rescale", _p(uncond_cond), float(guidance_scale), float(guidance_rescale), _p(out), rows, n_row, _s())
    return out


def sampler_step_rescaled(model_out, sample, guidance_scale, guidance_rescale, a0, a1, p, q, r=0.0, sigma=0.0, x0_prev=None,
                          noise=None, out=None, x0_out=None):
    """``sampler_step`` of the guided and rescaled model output in ONE launch: m' = ``cfg_rescale(model_out, guidance_scale,
    guidance_rescale)`` ; x0 = a0*m' + a1*sample ; out = p*sample + q*x0 + r*x0_prev + sigma*noise ; x0_out = x0.  ``model_out``
    is the stacked (2B, ...) [uncond | cond]; ``x0_prev`` may be None iff r == 0, ``noise`` iff sigma == 0.  ``out`` may be
    ``sample`` and ``x0_out`` may be ``x0_prev``; neither may overlap ``model_out``."""
    rows, n_row = _rescale_rows(model_out)
    assert sample.dtype == torch.float32 and sample.numel() == rows * n_row, (tuple(model_out.shape), tuple(sample.shape))
    for t in (x0_prev, noise, out, x0_out):
        assert t is None or (t.dtype == torch.float32 and t.numel() == sample.numel())
    if out is None:
        out = torch.empty_like(sample)
    L.call("mvd_op_sampler_step_rescaled", _p(model_out), float(guidance_scale), float(guidance_rescale), _p(sample), _p(x0_prev),
           _p(noise), float(a0), float(a1), float(p), float(q), float(r), float(sigma), _p(out), _p(x0_out), rows, n_row, _s())
    return out


def cfg_rescale_plan(n_row):
    """How the rescale kernel partitions a row of ``n_row`` floats (``mvd_debug_cfg_rescale_plan``): dict(threads, vec, wave, keep,
    passes) -- thread t of the row's one workgroup owns the ``vec``-float vectors t, t + threads, ...; ``keep`` vectors per thread
    stay in registers (0: the row is streamed twice); ``passes`` = vectors per thread."""
    out = (C.c_int * 4)()
    L.call("mvd_debug_cfg_rescale_plan", int(n_row), out)
    per_pass = out[0] * out[1]
    return dict(threads=out[0], vec=out[1], wave=out[2], keep=out[3], passes=-(-int(n_row) // per_pass))


def cfg_rescale_partition(n_row):
    """The element offsets in (0, n_row) at which the rescale kernel's partition of a row changes hands, sorted: every start of
    a wave's chunk (``wave * vec`` contiguous floats; a workgroup pass of ``threads * vec`` floats starts on one of them, and so
    does the last, partial pass), and every start of a lane's ``vec``-float chunk inside the first and the last wave chunk of the
    row -- the lane pattern repeats in every wave chunk, so the rest of them say nothing new.  Derived from the launcher's
    constants (``cfg_rescale_plan``)."""
    plan = cfg_rescale_plan(n_row)
    n_row, vec, wchunk = int(n_row), plan["vec"], plan["wave"] * plan["vec"]
    offs = set(range(wchunk, n_row, wchunk))
    offs.update(range(vec, min(wchunk, n_row), vec))
    last = (n_row - 1) // wchunk * wchunk
    offs.update(range(last + vec, n_row, vec))
    return sorted(offs)


APG_SPACES = ("output", "x0")                  # ``space`` of mvd_op_sampler_step_apg, by index


def _apg_momentum(momentum, momentum_buffer, rows, n_row):
    """The momentum buffer as the C entry gets it: required (the C side says so) when momentum != 0, not passed when it is 0."""
    if float(momentum) == 0.0 or momentum_buffer is None:
        return None
    if not (momentum_buffer.is_cuda and momentum_buffer.dtype == torch.float32 and momentum_buffer.is_contiguous()
            and momentum_buffer.numel() == rows * n_row):
        raise L.MvdError(f"apg: momentum_buffer must be a contiguous fp32 CUDA tensor of {rows} x {n_row} floats, got "
                         f"{tuple(momentum_buffer.shape)} {momentum_buffer.dtype} on {momentum_buffer.device}")
    return momentum_buffer


def apg(uncond_cond, guidance_scale, eta=0.0, norm_threshold=0.0, momentum=0.0, guidance_rescale=0.0, momentum_buffer=None,
        out=None):
    """(2B, ...) fp32 [uncond | cond] -> (B, ...): the guided output under adaptive projected guidance (Sadat et al., ICLR 2025;
    diffusers' ``normalized_guidance`` with ``use_original_formulation=True``), per batch row:
    d = (c - u) + momentum*M, M <- d ; s = min(1, norm_threshold / |d|) (0: no cap) ; m = c + (g - 1)*(s*d - (1 - eta)*par), par the
    part of s*d parallel to c ; then ``cfg_rescale``'s rescale when ``guidance_rescale`` > 0.  ``momentum_buffer`` (B, ...) fp32 is
    updated in place; it is required when ``momentum`` != 0 and untouched otherwise.  One launch (``mvd_op_apg``).  ``out`` and
    ``momentum_buffer`` must not overlap ``uncond_cond``."""
    rows, n_row = _rescale_rows(uncond_cond)
    if out is None:
        out = torch.empty((rows,) + tuple(uncond_cond.shape[1:]), device=uncond_cond.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() == rows * n_row and out.is_contiguous()
    L.call("mvd_op_apg", _p(uncond_cond), float(guidance_scale), float(eta), float(norm_threshold), float(momentum),
           float(guidance_rescale), _p(_apg_momentum(momentum, momentum_buffer, rows, n_row)), _p(out), rows, n_row, _s())
    return out


def sampler_step_apg(model_out, sample, guidance_scale, a0, a1, p, q, r=0.0, sigma=0.0, eta=0.0, norm_threshold=0.0, momentum=0.0,
                     guidance_rescale=0.0, space="output", momentum_buffer=None, x0_prev=None, noise=None, out=None, x0_out=None):
    """``sampler_step`` of the guided output under adaptive projected guidance in ONE launch: m = ``apg(model_out, ...)`` ;
    x0 = a0*m + a1*sample ; out = p*sample + q*x0 + r*x0_prev + sigma*noise ; x0_out = x0.  ``space="x0"`` (the paper's setting):
    the projection, the cap and the momentum buffer live in denoised-prediction space -- c <- a0*c + a1*sample, d <- a0*(c - u)
    first -- and m is the step's x0; ``guidance_rescale`` must then be 0.  ``model_out`` is the stacked (2B, ...) [uncond | cond];
    ``x0_prev`` may be None iff r == 0, ``noise`` iff sigma == 0, ``momentum_buffer`` iff momentum == 0.  ``out`` may be ``sample``
    and ``x0_out`` may be ``x0_prev``; no output may overlap ``model_out`` and ``momentum_buffer`` overlaps nothing."""
    rows, n_row = _rescale_rows(model_out)
    if space not in APG_SPACES:
        raise L.MvdError(f"sampler_step_apg: space={space!r}: expected one of {APG_SPACES}")
    assert sample.dtype == torch.float32 and sample.numel() == rows * n_row, (tuple(model_out.shape), tuple(sample.shape))
    for t in (x0_prev, noise, out, x0_out):
        assert t is None or (t.dtype == torch.float32 and t.numel() == sample.numel())
    if out is None:
        out = torch.empty_like(sample)
    L.call("mvd_op_sampler_step_apg", _p(model_out), float(guidance_scale), float(eta), float(norm_threshold), float(momentum),
           float(guidance_rescale), APG_SPACES.index(space), _p(_apg_momentum(momentum, momentum_buffer, rows, n_row)), _p(sample),
           _p(x0_prev), _p(noise), float(a0), float(a1), float(p), float(q), float(r), float(sigma), _p(out), _p(x0_out), rows, n_row,
           _s())
    return out


def apg_plan(n_row):
    """How the APG kernel partitions a row of ``n_row`` floats (``mvd_debug_apg_plan``): the dict of ``cfg_rescale_plan``."""
    out = (C.c_int * 4)()
    L.call("mvd_debug_apg_plan", int(n_row), out)
    per_pass = out[0] * out[1]
    return dict(threads=out[0], vec=out[1], wave=out[2], keep=out[3], passes=-(-int(n_row) // per_pass))


def unipc_step(model_out, sample, a0, a1, px, p0, p1=0.0, p2=0.0, corr=False, cx=0.0, c0=0.0, c1=0.0, c2=0.0, ct=0.0,
               last_sample=None, h0=None, h1=None, h2=None, guidance_scale=None, out=None, xc_out=None, x0_out=None):
    """fp32 UniPC step, corrector and predictor in ONE launch: m = model_out, or u + g*(c - u) of the stacked (2B, ...)
    [uncond | cond] when ``guidance_scale`` is given; x0 = a0*m + a1*sample ; xc = cx*last_sample + c0*h0 + c1*h1 + c2*h2 + ct*x0
    when ``corr``, else sample ; out = px*xc + p0*x0 + p1*h0 + p2*h1 ; xc_out = xc ; x0_out = x0.  ``h0`` .. ``h2`` are the previous
    x0 predictions, newest first; one whose coefficients are all 0 is not passed on (and may be None), ``last_sample`` goes only
    with ``corr``.  ``out`` may be ``sample``, ``xc_out`` may be ``last_sample`` and ``x0_out`` may be one of ``h0`` .. ``h2``; no
    output may overlap ``model_out``."""
    guided = guidance_scale is not None
    assert model_out.dtype == torch.float32 and sample.dtype == torch.float32
    assert model_out.numel() == sample.numel() * (2 if guided else 1), (tuple(model_out.shape), tuple(sample.shape))
    for t in (last_sample, h0, h1, h2, out, xc_out, x0_out):
        assert t is None or (t.dtype == torch.float32 and t.numel() == sample.numel())
    corr = bool(corr)
    if not corr:
        cx = c0 = c1 = c2 = ct = 0.0
    if out is None:
        out = torch.empty_like(sample)
    L.call("mvd_op_unipc_step", _p(model_out), int(guided), float(guidance_scale) if guided else 0.0, _p(sample),
           _p(last_sample if corr else None), _p(h0 if (c0 != 0.0 or p1 != 0.0) else None),
           _p(h1 if (c1 != 0.0 or p2 != 0.0) else None), _p(h2 if c2 != 0.0 else None), float(a0), float(a1), int(corr), float(cx),
           float(c0), float(c1), float(c2), float(ct), float(px), float(p0), float(p1), float(p2), _p(out), _p(xc_out), _p(x0_out),
           sample.numel(), _s())
    return out


def freeu(hidden, skip, H, W, b, s, hidden_out=None, skip_out=None):
    """FreeU (diffusers' ``apply_freeu``, threshold 1) on the two inputs of an up-block resnet, ONE launch (``mvd_op_freeu``).
    ``hidden`` (B, H*W, C) and ``skip`` (B, H*W, Cs) bf16, token-major -> ``(hidden', skip')``: channels [0, C // 2) of
    ``hidden`` times ``b`` (the rest bit for bit), and ``skip`` with its spatial frequencies {0, -1} x {0, -1} times ``s``.  The
    outputs must overlap neither input nor each other."""
    _bf16(hidden, skip, hidden_out, skip_out)
    if hidden.dim() != 3 or skip.dim() != 3 or hidden.shape[:2] != skip.shape[:2] or hidden.shape[1] != int(H) * int(W):
        raise L.MvdError(f"freeu: expected hidden (B, H*W, C) and skip (B, H*W, Cs) with H*W = {int(H) * int(W)}, got "
                         f"{tuple(hidden.shape)} and {tuple(skip.shape)}")
    if hidden_out is None:
        hidden_out = torch.empty_like(hidden)
    if skip_out is None:
        skip_out = torch.empty_like(skip)
    assert hidden_out.numel() == hidden.numel() and skip_out.numel() == skip.numel()
    L.call("mvd_op_freeu", _p(hidden), hidden.shape[2], _p(skip), skip.shape[2], hidden.shape[0], int(H), int(W), float(b), float(s),
           _p(hidden_out), _p(skip_out), _s())
    return hidden_out, skip_out


def _tome_shape(x, H, W, who):
    _bf16(x)
    if x.dim() != 3 or x.shape[1] != int(H) * int(W):
        raise L.MvdError(f"{who}: expected a (B, H*W, C) bf16 map with H*W = {int(H) * int(W)}, got {tuple(x.shape)}")


def tome_match(x, H, W, r, want_scores=False):
    """Token merging, the decisions (``mvd_op_tome_match``: the match and the select launch) for ``x`` (B, H*W, C) bf16 -- a block's
    LayerNorm1 output -- with ``r`` merged src per image.  Returns ``(slot, members, starts)`` int32 -- the merged row of every token
    (B, H*W), the tokens of every merged row in ascending order (B, H*W) and where each row's list starts (B, H*W - r + 1) -- and,
    with ``want_scores``, also ``(score, best)`` (B, #src) of every src token in ascending token order."""
    _tome_shape(x, H, W, "tome_match")
    B, HW, Cc = x.shape
    i32 = dict(dtype=torch.int32, device=x.device)
    slot, members = torch.empty(B, HW, **i32), torch.empty(B, HW, **i32)
    starts = torch.empty(B, max(HW - int(r), 0) + 1, **i32)
    ns = HW - (int(H) // 2) * (int(W) // 2)
    score = torch.empty(B, ns, dtype=torch.float32, device=x.device) if want_scores else None
    best = torch.empty(B, ns, **i32) if want_scores else None
    nws = 0 if want_scores else max(int(L.lib().mvd_op_tome_workspace_bytes(B, int(H), int(W))), 0)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
    L.call("mvd_op_tome_match", _p(x), B, int(H), int(W), Cc, int(r), _p(slot), _p(members), _p(starts), _p(score), _p(best), _p(ws), nws, _s())
    return (slot, members, starts, score, best) if want_scores else (slot, members, starts)


def tome_merge(x, H, W, r, members, starts, out=None):
    """The merged sequence (B, H*W - r, C) of ``x`` (B, H*W, C) bf16 under ``tome_match``'s tables (``mvd_op_tome_merge``): every row the
    fp32 mean of its members, summed in ascending token order, one rounding to bf16."""
    _tome_shape(x, H, W, "tome_merge")
    B, HW, Cc = x.shape
    assert members.dtype == torch.int32 and starts.dtype == torch.int32 and members.is_contiguous() and starts.is_contiguous()
    if out is None:
        out = torch.empty(B, max(HW - int(r), 0), Cc, dtype=torch.bfloat16, device=x.device)
    _bf16(out)
    if tuple(out.shape) != (B, HW - int(r), Cc) or tuple(members.shape) != (B, HW) or tuple(starts.shape) != (B, HW - int(r) + 1):
        raise L.MvdError(f"tome_merge: expected out {(B, HW - int(r), Cc)}, members {(B, HW)}, starts {(B, HW - int(r) + 1)}, got "
                         f"{tuple(out.shape)}, {tuple(members.shape)}, {tuple(starts.shape)}")
    L.call("mvd_op_tome_merge", _p(x), B, int(H), int(W), Cc, int(r), _p(members), _p(starts), _p(out), _s())
    return out


def tome_unmerge_add(h, t, H, W, r, slot):
    """``h`` (B, H*W, C) += ``t`` (B, H*W - r, C) rows by ``slot``, in place (``mvd_op_tome_unmerge_add``): bf16(float(h) + float(t))."""
    _tome_shape(h, H, W, "tome_unmerge_add")
    _bf16(t)
    B, HW, Cc = h.shape
    assert slot.dtype == torch.int32 and slot.is_contiguous() and tuple(slot.shape) == (B, HW)
    if tuple(t.shape) != (B, HW - int(r), Cc):
        raise L.MvdError(f"tome_unmerge_add: expected t {(B, HW - int(r), Cc)}, got {tuple(t.shape)}")
    L.call("mvd_op_tome_unmerge_add", _p(h), _p(t), B, int(H), int(W), Cc, int(r), _p(slot), _s())
    return h


def tome_plan(H, W, C_, r):
    """What the token-merging kernels do with an H x W map of C_ channels and r merged src (``mvd_debug_tome_plan``); MvdError, with
    ``max_tokens`` in the message, for a shape they refuse."""
    out = (C.c_int64 * 8)()
    L.call("mvd_debug_tome_plan", int(H), int(W), int(C_), int(r), out)
    return dict(dst=out[0], src=out[1], rows=out[2], score_keys=out[3], member_keys=out[4], match_workgroups=out[5], select_lds=out[6],
                max_tokens=out[7])


TODO_METHODS = ("nearest", "area")          # method of mvd_op_todo_downsample, by index


def todo_downsample(qkv_or_k, v, H, W, f, method, out=None, channels=None):
    """Token downsampling of K and V rows (``mvd_op_todo_downsample``, one launch): the keys and values of an ``H`` x ``W`` token map
    pooled by the factor ``f`` into ``out`` (B, (H // f) * (W // f), 2C) bf16, K in columns ``[0, C)`` and V in ``[C, 2C)``.
    ``method``: ``"nearest"`` (the top-left token of every complete f x f cell, bit for bit) or ``"area"`` (the cell's mean: fp32 sum
    in row-major order, divided by f*f, one rounding to bf16); 0 / 1 are taken too.
    ``qkv_or_k`` and ``v`` are the K and V columns, (B, H*W, C) views with a shared row stride (slices of the fused q/k/v rows:
    ``qkv[..., C:2*C]`` and ``qkv[..., 2*C:3*C]``).  With ``v=None`` the first argument is the fused (B, H*W, 3C or 4C) buffer itself,
    q | k | v [| q_ref], of ``channels`` channels (default: a third of its width)."""
    if v is None:
        qkv = qkv_or_k
        _bf16(qkv)
        Cc = int(channels) if channels is not None else qkv.shape[-1] // 3
        if qkv.dim() != 3 or qkv.shape[-1] < 3 * Cc or Cc <= 0:
            raise L.MvdError(f"todo_downsample: expected fused (B, H*W, >= 3C) q/k/v rows, got {tuple(qkv.shape)} with C = {Cc}")
        k, v = qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:3 * Cc]
    else:
        k = qkv_or_k
    for t in (k, v):
        if t.dtype != torch.bfloat16 or not t.is_cuda or t.dim() != 3:
            raise L.MvdError(f"todo_downsample: k and v must be (B, H*W, C) bf16 tensors on the GPU, got {t.dtype} {tuple(t.shape)}")
    B, HW, Cc = k.shape
    if tuple(v.shape) != (B, HW, Cc) or HW != int(H) * int(W):
        raise L.MvdError(f"todo_downsample: expected k and v (B, {int(H) * int(W)}, C), got {tuple(k.shape)} and {tuple(v.shape)}")
    ld = k.stride(1)
    if k.stride(2) != 1 or v.stride() != k.stride() or (B > 1 and k.stride(0) != HW * ld):
        raise L.MvdError(f"todo_downsample: k and v must share a row stride and the batch stride H*W*ld, got strides {k.stride()} and {v.stride()}")
    m = TODO_METHODS.index(method) if method in TODO_METHODS else method
    if isinstance(m, bool) or not isinstance(m, int):
        raise L.MvdError(f"todo_downsample: method must be one of {TODO_METHODS}, got {method!r}")
    fi = int(f)
    Nk = (int(H) // fi) * (int(W) // fi) if fi > 0 else 0
    if out is None:
        out = torch.empty(B, max(Nk, 1), 2 * Cc, dtype=torch.bfloat16, device=k.device)
        if Nk < 1:
            out = out[:, :0]
    _bf16(out)
    if Nk >= 1 and tuple(out.shape) != (B, Nk, 2 * Cc):
        raise L.MvdError(f"todo_downsample: expected out {(B, Nk, 2 * Cc)}, got {tuple(out.shape)}")
    L.call("mvd_op_todo_downsample", C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), int(ld), B, int(H), int(W), Cc, fi, int(m), _p(out), _s())
    return out


PREDICTION_TYPES = ("epsilon", "v_prediction", "sample")       # prediction_type of mvd_op_noise_loss, by index


def _f32_same(*ts):
    first = next(t for t in ts if t is not None)
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == first.shape):
            raise L.MvdError(f"expected contiguous fp32 CUDA tensors of shape {tuple(first.shape)}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")


def _timesteps_i32(timesteps, batch, device):
    t = torch.as_tensor(timesteps, device=device)
    if t.dim() == 0:
        t = t.expand(batch)
    if t.dim() != 1 or t.shape[0] != batch or t.is_floating_point():
        raise L.MvdError(f"timesteps: expected {batch} integers, got {t.dtype} {tuple(t.shape)}")
    return t.to(torch.int32).contiguous()


def add_noise(x0, noise, timesteps, sqrt_ac, sqrt_1mac, noisy=True, velocity=False):
    """fp32 (B, ...): noisy = a*x0 + s*noise and / or velocity = a*noise - s*x0 with a = sqrt_ac[t_b], s = sqrt_1mac[t_b]; the
    tables are fp32 device vectors, ``timesteps`` B integers (a device tensor is not range-checked: no sync).  Returns
    (noisy or None, velocity or None)."""
    _f32_same(x0, noise)
    b = x0.shape[0]
    ts = _timesteps_i32(timesteps, b, x0.device)
    assert sqrt_ac.dtype == torch.float32 and sqrt_1mac.dtype == torch.float32 and sqrt_ac.numel() == sqrt_1mac.numel()
    yn = torch.empty_like(x0) if noisy else None
    yv = torch.empty_like(x0) if velocity else None
    L.call("mvd_op_add_noise", _p(x0), _p(noise), _p(ts), _p(sqrt_ac), _p(sqrt_1mac), sqrt_ac.numel(), _p(yn), _p(yv), b,
           x0.numel() // b, _s())
    return yn, yv


def noise_loss(pred, noise, timesteps, sqrt_ac, sqrt_1mac, snr, prediction_type="v_prediction", x0=None, noisy=None,
               snr_gamma=5.0, want_denoised=False):
    """One pass over (pred, noise, x0, noisy), fp32 (B, ...): returns (result, denoised or None) with the device vector
    result = [mse(pred, target), mse * mean_b(min(snr_b, gamma) / snr_b), mse(denoised, x0), mean_b snr_b, mean_b weight_b]
    (mvd_hip.h has the formulas per ``prediction_type``).  Nothing is synchronised or uploaded."""
    _f32_same(pred, noise, x0, noisy)
    if prediction_type not in PREDICTION_TYPES:
        raise L.MvdError(f"prediction_type={prediction_type!r}: expected one of {PREDICTION_TYPES}")
    b = pred.shape[0]
    per = pred.numel() // b
    ts = _timesteps_i32(timesteps, b, pred.device)
    for t in (sqrt_ac, sqrt_1mac, snr):
        assert t.dtype == torch.float32 and t.numel() == sqrt_ac.numel()
    nbytes = L.check(L.lib().mvd_op_noise_loss_ws_bytes(b, per), "mvd_op_noise_loss_ws_bytes")
    ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    result = torch.empty(5, device=pred.device, dtype=torch.float32)
    den = torch.empty_like(pred) if want_denoised else None
    L.call("mvd_op_noise_loss", _p(pred), _p(noise), _p(x0), _p(noisy), _p(ts), _p(sqrt_ac), _p(sqrt_1mac), _p(snr), sqrt_ac.numel(),
           PREDICTION_TYPES.index(prediction_type), float(snr_gamma), _p(den), _p(result), b, per, _p(ws), nbytes, _s())
    return result, den


def image_metrics(x, y, data_range, ssim=True, per_image=False):
    """fp32 NCHW batches: returns (result, per-image or None) with the device vectors result = [mse, ssim, psnr] and
    per-image (N, 2) = each image's (mse, ssim).  SSIM as pytorch_msssim 1.0.0's defaults, PSNR = 10 log10(R^2 / mse)
    (mvd_hip.h); ``ssim=False`` leaves result[1] = 0.  H, W >= 11."""
    _f32_same(x, y)
    if x.dim() != 4:
        raise L.MvdError(f"image_metrics: expected (N, C, H, W), got {tuple(x.shape)}")
    n, c, h, w = x.shape
    nbytes = L.check(L.lib().mvd_op_image_metrics_ws_bytes(n, c, h, w, int(ssim)), "mvd_op_image_metrics_ws_bytes")
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    result = torch.empty(3, device=x.device, dtype=torch.float32)
    pi = torch.empty(n, 2, device=x.device, dtype=torch.float32) if per_image else None
    L.call("mvd_op_image_metrics", _p(x), _p(y), n, c, h, w, float(data_range), int(ssim), _p(result), _p(pi), _p(ws), nbytes, _s())
    return result, pi


def _rows(t):
    """(pointer, row stride) of a 2-D fp32 CUDA tensor whose rows are dense: a column slice or an offset view of a wider
    buffer is passed as it is, its ``stride(0)`` as the leading dimension."""
    assert t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), "rows must be dense fp32"
    return C.c_void_p(t.data_ptr()), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def skinny_linear(x, w, bias=None, silu_in=False, out=None):
    """fp32 linear layer of the camera / time MLPs: x (B, K) fp32, w (N, K) fp32 or bf16 -> (B, N) fp32.  ``x`` may be a view with
    ``stride(0) > K`` (ldx); ``out`` a (B, N) view of a wider buffer, ``stride(0)`` its ldy (the engine writes the two halves of
    its concatenated input that way) -- the columns of the buffer outside the view are not written."""
    assert x.dim() == 2 and w.dim() == 2 and w.shape[1] == x.shape[1]
    assert w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous()
    b, k = x.shape
    n = w.shape[0]
    y = torch.empty(b, n, device=x.device, dtype=torch.float32) if out is None else out
    assert tuple(y.shape) == (b, n)
    (xp, ldx), (yp, ldy) = _rows(x), _rows(y)
    L.call("mvd_op_skinny_linear", xp, ldx, b, k, _p(w), int(w.dtype == torch.bfloat16), _p(bias), n, int(silu_in), yp, ldy, _s())
    return y


def _seg(seg_end):
    return (C.c_int * len(seg_end))(*[int(v) for v in seg_end]), len(seg_end)


def skinny_linear_grouped(x, w, seg_end, bias=None, xseg=None):
    """x (B, nseg * K) fp32 (or any row-dense view; segment g's input row starts ``g * xseg`` floats in, default K), w (N, K) fp32,
    ``seg_end``: the ends of the output-feature segments (the last one N) -> (B, N) fp32."""
    assert w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and x.dim() == 2
    n, k = w.shape
    b = x.shape[0]
    y = torch.empty(b, n, device=x.device, dtype=torch.float32)
    xp, ldx = _rows(x)
    se, ns = _seg(seg_end)
    xseg = k if xseg is None else int(xseg)
    assert xseg >= 0 and (ns - 1) * xseg + k <= x.shape[1] and (bias is None or bias.numel() == n), "a segment's input lies outside the row"
    L.call("mvd_op_skinny_linear_grouped", xp, ldx, xseg, b, k, _p(w), _p(bias), n, se, ns, _p(y), n, _s())
    return y


def timestep_embedding(t, dim):
    """t (B,) fp32 -> (B, dim) fp32 [cos | sin] (diffusers ``Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0)``)."""
    assert t.dtype == torch.float32 and t.dim() == 1
    y = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
    L.call("mvd_op_timestep_embedding", _p(t), t.shape[0], int(dim), _p(y), _s())
    return y


def camera_features(src, tgt, nfreq, max_freq=10.0):
    """cameras (B, 3 or 4, 4) fp32 -> (rflat (B, 9), enc (B, 6 * nfreq)): the relative rotation and the Fourier features of the
    relative translation, per axis [sin nfreq | cos nfreq]."""
    assert src.dtype == torch.float32 and tgt.dtype == torch.float32 and src.shape == tgt.shape and src.dim() == 3 and src.shape[2] == 4
    b, rows = src.shape[0], src.shape[1]
    rflat = torch.empty(b, 9, device=src.device, dtype=torch.float32)
    enc = torch.empty(b, 6 * nfreq, device=src.device, dtype=torch.float32)
    L.call("mvd_op_camera_features", _p(src), _p(tgt), b, rows, int(nfreq), float(max_freq), _p(rflat), _p(enc), _s())
    return rflat, enc


def layernorm_f32(x, gamma, beta, eps=1e-5, silu=False, nseg=1):
    """x (rows, c) fp32; gamma / beta (c,) or, grouped, (nseg, c): row r takes the affine of segment r % nseg."""
    assert x.dtype == torch.float32 and x.dim() == 2 and gamma.numel() == nseg * x.shape[1] and beta.numel() == nseg * x.shape[1]
    y = torch.empty_like(x)
    L.call("mvd_op_layernorm_f32", _p(x), x.shape[0], x.shape[1], float(eps), _p(gamma), _p(beta), int(silu), int(nseg), _p(y), _s())
    return y


def film_params(raw, strength, out_rows=None):
    """raw (B, 2 * dim) fp32 -> (scale, shift), (out_rows, dim) each; output row r comes from raw row r % B."""
    assert raw.dtype == torch.float32 and raw.dim() == 2 and raw.shape[1] % 2 == 0
    b, dim = raw.shape[0], raw.shape[1] // 2
    rows = b if out_rows is None else int(out_rows)
    scale = torch.empty(rows, dim, device=raw.device, dtype=torch.float32)
    shift = torch.empty(rows, dim, device=raw.device, dtype=torch.float32)
    L.call("mvd_op_film_params", _p(raw), b, dim, float(strength), _p(scale), _p(shift), rows, _s())
    return scale, shift


def film_params_grouped(raw, seg_end, strength, out_rows=None):
    """raw (B, seg_end[-1]) fp32, segment g holding 2 * dim_g features -> the flat engine layout (out_rows * seg_end[-1],): per
    segment scale (out_rows, dim_g) | shift (out_rows, dim_g)."""
    assert raw.dtype == torch.float32 and raw.dim() == 2 and raw.shape[1] == seg_end[-1]
    b = raw.shape[0]
    rows = b if out_rows is None else int(out_rows)
    out = torch.empty(rows * seg_end[-1], device=raw.device, dtype=torch.float32)
    se, ns = _seg(seg_end)
    L.call("mvd_op_film_params_grouped", _p(raw), b, se, ns, float(strength), _p(out), rows, _s())
    return out


def im2col_in(x, scale=None, shift=None, ld_ss=0):
    """x (B, C, H, W) fp32, C <= 7 (+ FiLM ``x * scale[b * ld_ss + ch] + shift[b * ld_ss + ch]``) -> (B, H, W, 64) bf16 rows of the
    3x3 pad-1 window, column tap * C + ch."""
    assert x.dtype == torch.float32 and x.dim() == 4
    B, c, H, W = x.shape
    if scale is not None:
        need = (B - 1) * ld_ss + c
        assert scale.dtype == torch.float32 and shift.dtype == torch.float32 and scale.numel() >= need and shift.numel() >= need
    y = torch.empty(B, H, W, 64, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_im2col_in", _p(x), B, c, H, W, _p(scale), _p(shift), int(ld_ss), _p(y), _s())
    return y


def film_nchw_f32(x, scale, shift):
    """x (B, C, HW) fp32, scale / shift (B, C) fp32 -> x * scale + shift."""
    assert x.dtype == torch.float32 and x.dim() == 3 and tuple(scale.shape) == tuple(x.shape[:2]) == tuple(shift.shape)
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    y = torch.empty_like(x)
    L.call("mvd_op_film_nchw_f32", _p(x), x.shape[0], x.shape[1], x.shape[2], _p(scale), _p(shift), _p(y), _s())
    return y


def nchw_to_nhwc(x, scale=None, shift=None):
    B, c, H, W = x.shape
    y = torch.empty(B, H, W, c, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_nchw_to_nhwc", _p(x), B, c, H * W, _p(scale), _p(shift), _p(y), _s())
    return y


def nhwc_to_nchw(x):
    """x (B, H, W, C) bf16 -> (B, C, H, W) fp32 (the engine's output layout change)."""
    _bf16(x)
    B, H, W, c = x.shape
    y = torch.empty(B, c, H, W, device=x.device, dtype=torch.float32)
    L.call("mvd_op_nhwc_to_nchw", _p(x), B, H * W, c, _p(y), _s())
    return y


def f32_to_bf16(x):
    """fp32 tensor -> bf16 of the same shape, round to nearest even."""
    assert x.dtype == torch.float32
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    L.call("mvd_op_f32_to_bf16", _p(x), x.numel(), _p(y), _s())
    return y


def last_gemm_plan():
    """dict(cfg, splitk, tiles, grid, per_cu) of this thread's last GEMM / conv launch."""
    out = (C.c_int * 5)()
    L.call("mvd_debug_last_gemm_plan", out)
    return dict(cfg=out[0], splitk=out[1], tiles=out[2], grid=out[3], per_cu=out[4], nowait=L.lib().mvd_debug_last_gemm_nowait())


def last_attention_plan():
    out = (C.c_int * 2)()
    L.call("mvd_debug_last_attention_plan", out)
    return dict(waves=out[0], workgroups=out[1])


def last_groupnorm_plan():
    """This thread's last GroupNorm launch.  One-pass slice kernel: dict(form="slice", nv, threads, gpw, npl) -- the instantiation's
    vectors per thread, groups per workgroup, pixels per pass; two-kernel form: dict(form="two_kernel", R, threads, nchunk,
    rows_per_chunk, apply_rows) -- rows in flight of gn_stats, its chunks per image, and gn_apply's rows per block."""
    out = (C.c_int * 6)()
    L.call("mvd_debug_last_groupnorm_plan", out)
    if out[0] == 1:
        return dict(form="slice", nv=out[1], threads=out[2], gpw=out[3], npl=out[4])
    if out[0] == 2:
        return dict(form="two_kernel", R=out[1], threads=out[2], nchunk=out[3], rows_per_chunk=out[4], apply_rows=out[5])
    return dict(form="none")


def engine_splitk(m, n, k, geglu=False, conv=False):
    """The split-K factor the engine's schedule uses for this GEMM (or, ``conv=True``, 3x3 convolution) size."""
    if conv:
        return L.lib().mvd_debug_pick_splitk_conv(m, n, k)
    return L.lib().mvd_debug_pick_splitk(m, n, k, int(geglu))


def engine_dense_route(m, n, k1, k2=0):
    """The route the engine's single-stream schedule gives a dense GEMM ``[a | a2] @ w.T`` (+ bias, residual) of this size, from
    host arithmetic alone (no GPU needed): dict(sm, cfg, splitk, depth, walk_cg, force_cfg) -- ``sm``: the small-M kernels take it
    (``cfg`` is then their tile and ``depth`` the ring depth); ``force_cfg``: what ``linear(..., force_cfg=, splitk=)`` needs to
    run that route (-1: the tiled kernels' own heuristic)."""
    out = (C.c_int * 5)()
    L.call("mvd_debug_dense_route", m, n, k1, k2, out)
    sm = bool(out[0])
    return dict(sm=sm, cfg=out[1], splitk=out[2], depth=out[3], walk_cg=out[4], force_cfg=100 + 10 * out[1] + out[3] if sm else -1)
