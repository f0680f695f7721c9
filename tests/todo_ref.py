"""Token downsampling of the self-attention keys (ToDo), restated on the CPU -- the definition the
operator and the engine are held to (tests/test_todo_cpu.py pins it against ``F.interpolate`` / ``F.avg_pool2d``).

(a) geometry: the key map of an H x W token map under a factor f is Hk x Wk = (H // f) x (W // f); tokens of an incomplete last row
    or column of cells are queries but never keys.
(b) ``downsample``: ``nearest`` -- key (i, j) is token (i f, j f); ``area`` -- the mean of the f x f cell.  On bf16 rows the mean is
    the kernel's: the f*f values summed in fp32 in row-major order inside the cell, one fp32 division by float(f*f), one rounding to
    bf16 (RNE).  On fp32 / fp64 rows (the oracle) it is the same sum in that type.
(c) ``reference_kv``: the operator's output for a fused q/k/v buffer, with the op-level faults of ``OP_FAULTS`` on request.
(d) ``todo_oracle``: the oracle forward with attn1's keys and values taken from the downsampled LayerNorm rows in the eligible
    main-pass blocks, with the wrong-on-purpose variants of ``ORACLE_WRONG``."""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import sd21_unet as OU

METHODS = ("nearest", "area")
PARITY_BOUND_MAX = 3e-2           # the cap on the engine parity bound (tests/test_todo_cpu.py: every wrong variant is >= 4 x this away)
PARITY_SETTING = dict(factor=2, factor_level_2=1, method="nearest")


# ------------------------------------------------------------------------------------------------------------- (a) geometry
def key_grid(H, W, f):
    """(Hk, Wk, Nk)"""
    return H // f, W // f, (H // f) * (W // f)


def cell_tokens(H, W, f, *, col_off=0, include_incomplete=False):
    """(Nk, f*f) token indices of every cell in row-major order inside the cell, and a (Nk, f*f) mask of the entries that exist.
    WRONG on purpose: ``col_off`` shifts every cell by that many columns (clamped to the map); ``include_incomplete`` adds the
    cells of an incomplete last row / column."""
    Hk, Wk = (-(-H // f), -(-W // f)) if include_incomplete else (H // f, W // f)
    i = torch.arange(Hk)[:, None, None, None] * f + torch.arange(f)[None, None, :, None]
    j = torch.arange(Wk)[None, :, None, None] * f + torch.arange(f)[None, None, None, :] + col_off
    ok = (i < H) & (j < W) & (j >= 0)
    ok = ok.expand(Hk, Wk, f, f)
    idx = (i.clamp(max=H - 1) * W + j.clamp(0, W - 1)).expand(Hk, Wk, f, f)
    return idx.reshape(Hk * Wk, f * f), ok.reshape(Hk * Wk, f * f)


def block_factor(latent_hw, H, W, factor, factor_level_2):
    """the factor of a block whose map is H x W at a latent of latent_hw; 1: untouched"""
    down = math.ceil(math.sqrt((latent_hw[0] * latent_hw[1]) // (H * W)))
    f = factor if down == 1 else factor_level_2 if down == 2 else 1
    return f if f > 1 and H // f >= 1 and W // f >= 1 else 1


# ------------------------------------------------------------------------------------------------------- (b) the definition
def truncate_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (WRONG: the kernel rounds to nearest even)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def downsample(x, H, W, f, method, *, corner=False, col_off=0, include_incomplete=False, reverse_sum=False, truncate=False):
    """x (B, H*W, C) -> (B, Nk, C) in x's dtype.  WRONG on purpose: ``corner`` -- nearest takes the bottom-right token of the cell;
    ``col_off`` / ``include_incomplete`` -- see ``cell_tokens``; ``reverse_sum`` -- the cell is summed last token first;
    ``truncate`` -- bf16 by truncation."""
    assert method in METHODS and x.dim() == 3 and x.shape[1] == H * W
    idx, ok = cell_tokens(H, W, f, col_off=col_off, include_incomplete=include_incomplete)
    if method == "nearest":
        return x[:, idx[:, -1 if corner else 0]]
    acc_t = torch.float32 if x.dtype == torch.bfloat16 else x.dtype
    order = range(f * f - 1, -1, -1) if reverse_sum else range(f * f)
    acc = None
    for p in order:                                   # one correctly rounded addition per member, in this order
        term = x[:, idx[:, p]].to(acc_t) * ok[:, p, None].to(acc_t)
        acc = term if acc is None else acc + term
    cnt = ok.sum(dim=1).to(acc_t)[None, :, None] if include_incomplete else torch.tensor(float(f * f), dtype=acc_t)
    mean = acc / cnt
    if x.dtype != torch.bfloat16:
        return mean
    return truncate_bf16(mean) if truncate else mean.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- (c) the operator and its faults
OP_FAULTS = {
    "corner": dict(corner=True),                          # (nearest only: area has no corner)
    "cell off by one column": dict(col_off=1),
    "incomplete last cell included": dict(include_incomplete=True),       # (maps with H % f or W % f only)
    "sum order reversed": dict(reverse_sum=True),         # (area only; the planted "cancel" inputs tell it apart)
    "truncation for RNE": dict(truncate=True),            # (area only)
    "V from K's columns": dict(v_from_k=True),
    "batch stride hw*C for hw*ld": dict(short_batch_stride=True),         # (B > 1 only)
}


def reference_kv(qkv, C, H, W, f, method, *, v_from_k=False, short_batch_stride=False, **wrong):
    """The operator's output (B, Nk, 2C) bf16 for fused rows ``qkv`` (B, H*W, ld) bf16, q | k | v [| q_ref]."""
    B, HW, ld = qkv.shape
    src = qkv
    if short_batch_stride:                                # image b starts hw*C elements after image b - 1 (clamped to the buffer)
        flat = qkv.reshape(-1)
        start = (torch.arange(B) * HW * C).clamp(max=flat.numel() - HW * ld)
        src = torch.stack([flat[int(s):int(s) + HW * ld].reshape(HW, ld) for s in start])
    k = src[..., C:2 * C]
    v = k if v_from_k else src[..., 2 * C:3 * C]
    return torch.cat([downsample(k, H, W, f, method, **wrong), downsample(v, H, W, f, method, **wrong)], dim=-1)


# (B, H, W, C, f): one cell map, a batch, odd in both directions, factor 3, factor 4 with a remainder, several workgroups, one key
OP_CASES = [(1, 8, 8, 320, 2), (3, 6, 10, 320, 2), (2, 7, 9, 640, 2), (2, 7, 10, 320, 3), (1, 9, 9, 1280, 4), (2, 16, 16, 1280, 2), (1, 4, 4, 64, 4)]
OP_WIDTHS = (3, 4)                # ld = 3C and 4C
OP_INPUTS = ("gauss", "int", "cancel")


def case_id(c):
    return "B{}_{}x{}_C{}_f{}".format(*c)


def fused_rows(case, width, kind, seed=0):
    """(B, H*W, width*C) bf16 fused rows.  ``gauss``: N(0, 1); ``int``: integers in [-8, 8] (every sum exact); ``cancel``: small
    integers with +L and -L (L = 2^25) planted at two random positions of every cell and channel -- what is added between the two
    is lost to fp32 rounding, so the cell's sum depends on the ORDER of the additions."""
    B, H, W, C, f = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + C + f + width)
    shape = (B, H * W, width * C)
    if kind == "gauss":
        return torch.randn(shape, generator=g).to(torch.bfloat16)
    x = torch.randint(-8, 9, shape, generator=g).float()
    if kind == "cancel":
        x = torch.randint(1, 4, shape, generator=g).float()
        idx, _ = cell_tokens(H, W, f)
        Nk = idx.shape[0]
        pick = torch.rand((B, Nk, f * f, width * C), generator=g).argsort(dim=2)[:, :, :2]        # two distinct positions per cell and channel
        for s, val in ((0, 2.0 ** 25), (1, -2.0 ** 25)):
            tok = idx[torch.arange(Nk)[None, :, None], pick[:, :, s]]                             # (B, Nk, width*C) token index
            x.scatter_(1, tok, torch.full(tok.shape, val))
    return x.to(torch.bfloat16)


def check_op(out, qkv, case, method, **fault_free):
    """the operator checks of tests/test_todo_ops_gpu.py: shape, and K and V each against their own columns, bit for bit"""
    B, H, W, C, f = case
    want = reference_kv(qkv, C, H, W, f, method)
    assert tuple(out.shape) == tuple(want.shape), (tuple(out.shape), tuple(want.shape))
    assert torch.equal(out[..., :C], want[..., :C]), "K"
    assert torch.equal(out[..., C:], want[..., C:]), "V"


# ------------------------------------------------------------------------------------------------ the engine tests' inputs
PERIOD2_ABOVE_KEYS = 128          # level-0 key maps (factor 2) above this get the period-2 component below
PERIOD2_AMPLITUDE = 1.0


def parity_inputs(cfg, batch, hw, seed=0):
    """``parity_util.make_inputs(cfg, batch, hw, 7, seed, 96)``; for a latent whose level-0 key map under factor 2 has more than
    ``PERIOD2_ABOVE_KEYS`` keys (of the engine cases: 48 x 48, 576 keys) the sample gets a zero-mean component of period 2 added:
    +A on the tokens with even row and even column -- the ones ``nearest`` keeps -- and -A / 3 on the others.
    Why: ``make_inputs`` draws the sample as white noise, under which self-attention with seeded weights is close to a mean over the
    keys, and a mean over every fourth key differs from the mean over all of them like a Monte-Carlo error, ~ 1 / sqrt(Nk).  On the
    ORACLE alone (CPU, seeds 0..3, rel-L2 of its ToDo result to its plain result): 1.9e-1 at 64 keys (16 x 16), 1.4e-1 at 128
    (16 x 32), 8.6e-2 .. 1.0e-1 at 256 (32 x 32), 5.6e-2 .. 7.9e-2 at 576 (48 x 48, sixteen seeds) -- at 48 x 48 white noise leaves
    downsampling on and off closer than four parity bounds whatever computes them, so a forward that ignored the switch could not
    be told from one that honours it.  With the component the kept tokens differ from the dropped ones systematically: 2.7e-1 at
    48 x 48 (tests/test_todo_cpu.py asserts at least 4 x PARITY_BOUND_MAX there, on the oracle).  The parity bound is measured on
    these same inputs with the switch off, as for every case."""
    from tests.parity_util import make_inputs
    inp = make_inputs(cfg, batch, hw, 7, seed, 96)
    h, w = (hw, hw) if isinstance(hw, int) else hw
    if (h // 2) * (w // 2) > PERIOD2_ABOVE_KEYS:
        even = ((torch.arange(h)[:, None] % 2 == 0) & (torch.arange(w)[None, :] % 2 == 0)).float()
        inp["sample"] = inp["sample"] + PERIOD2_AMPLITUDE * (even - (1.0 - even) / 3.0)
    return inp


# ------------------------------------------------------------------------------------------------------ (d) the ToDo oracle
ORACLE_WRONG = ("levels_shift", "corner", "also_ref", "factor_off", "swap_method")


@contextlib.contextmanager
def todo_oracle(factor=2, factor_level_2=1, method="nearest", *, levels_shift=0, corner=False, also_ref=False, factor_off=False,
                swap_method=False, record=None, latent_hw=None):
    """Inside the block every MAIN-pass oracle forward (the forwards that do not pass ``capture``) runs ``attn1`` of the eligible
    transformer blocks as ``attention(n, ctx=downsample(n))``: every query, the keys and values of the downsampled LayerNorm rows.
    The adapter's "self" hook gets the full ``n``; everything else is the plain block.  ``record``: a dict that receives
    ``{feature name: Nk}``.  ``latent_hw``: the latent size of a ``transformer_2d`` call made OUTSIDE ``unet_forward`` (one block
    on its own, tests/block_ref.py); inside a forward the forward's own sample decides, as ever.  Yields ``pool_ref``: what the
    reference feature map (Br, C, H, W) behind the adapter's self branch becomes -- itself, but for ``also_ref`` inside the self hook
    of a downsampled block (a hook that does not go through ``oracle.mvd.image_cross_attention`` asks it).
    WRONG on purpose: ``levels_shift`` -- the level rule sees a latent 2^shift times coarser per side (the blocks of THAT level take
    ``factor``, the level below ``factor_level_2``, the finer ones nothing); ``corner`` -- nearest takes the cell's bottom-right token; ``also_ref`` -- the reference feature map behind the adapter's self
    branch is downsampled the same way, so the reference K/V are pooled too; ``factor_off`` -- f + 1; ``swap_method`` -- the other method."""
    from oracle import mvd as OM
    orig_forward, orig_tf, orig_ica = OU.unet_forward, OU.transformer_2d, OM.image_cross_attention
    state = {"latent": None if latent_hw is None else tuple(latent_hw), "ref_pool": None}      # (outside a forward)
    meth = METHODS[1 - METHODS.index(method)] if swap_method else method

    def forward(p, cfg, sample, timestep, text, attn_hook=None, block_hook=None, capture=None, **kw):
        prev = state["latent"]
        state["latent"] = tuple(sample.shape[-2:]) if capture is None else None
        try:
            return orig_forward(p, cfg, sample, timestep, text, attn_hook=attn_hook, block_hook=block_hook, capture=capture, **kw)
        finally:
            state["latent"] = prev

    def pool_ref(ref_nchw):
        if state["ref_pool"] is not None:
            fr, Br, Cr, Hr, Wr = (state["ref_pool"],) + tuple(ref_nchw.shape)
            rows = downsample(ref_nchw.permute(0, 2, 3, 1).reshape(Br, Hr * Wr, Cr), Hr, Wr, fr, meth, corner=corner)
            ref_nchw = rows.reshape(Br, Hr // fr, Wr // fr, Cr).permute(0, 3, 1, 2)
        return ref_nchw

    def ref_attention(w, hidden, ref_nchw, heads, *a, **kw):
        return orig_ica(w, hidden, pool_ref(ref_nchw), heads, *a, **kw)

    def transformer(p, key, x, text, heads, groups, attn_hook, hook_name):
        lat = state["latent"]
        B, C, H, W = x.shape
        f = 1
        if lat is not None:
            see = (max(lat[0] >> levels_shift, 1), max(lat[1] >> levels_shift, 1))
            f = block_factor(see, H, W, factor, factor_level_2)
            if f > 1 and factor_off:
                f = f + 1 if H // (f + 1) >= 1 and W // (f + 1) >= 1 else f
        if f <= 1:
            return orig_tf(p, key, x, text, heads, groups, attn_hook, hook_name)
        N = H * W
        res = x
        h = OU._gn(x, p, f"{key}.norm", groups, 1e-6)
        h = h.permute(0, 2, 3, 1).reshape(B, N, C)
        h = F.linear(h, p[f"{key}.proj_in.weight"], p[f"{key}.proj_in.bias"])
        b = f"{key}.transformer_blocks.0"
        n = F.layer_norm(h, (C,), p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], 1e-5)
        ctx = downsample(n, H, W, f, meth, corner=corner)
        if record is not None:
            record[hook_name] = ctx.shape[1]
        a = OU.attention(p, f"{b}.attn1", n, ctx, heads)
        if attn_hook is not None:
            state["ref_pool"] = f if also_ref else None
            try:
                a = attn_hook(hook_name, "self", n, a)
            finally:
                state["ref_pool"] = None
        h = h + a
        n = F.layer_norm(h, (C,), p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], 1e-5)
        a = OU.attention(p, f"{b}.attn2", n, text, heads)
        if attn_hook is not None:
            a = attn_hook(hook_name, "cross", n, a)
        h = h + a
        n = F.layer_norm(h, (C,), p[f"{b}.norm3.weight"], p[f"{b}.norm3.bias"], 1e-5)
        ff = F.linear(n, p[f"{b}.ff.net.0.proj.weight"], p[f"{b}.ff.net.0.proj.bias"])
        val, gate = ff.chunk(2, dim=-1)
        ff = F.linear(val * F.gelu(gate), p[f"{b}.ff.net.2.weight"], p[f"{b}.ff.net.2.bias"])
        h = h + ff
        h = F.linear(h, p[f"{key}.proj_out.weight"], p[f"{key}.proj_out.bias"])
        return h.reshape(B, H, W, C).permute(0, 3, 1, 2) + res

    OU.unet_forward, OU.transformer_2d, OM.image_cross_attention = forward, transformer, ref_attention
    try:
        yield pool_ref
    finally:
        OU.unet_forward, OU.transformer_2d, OM.image_cross_attention = orig_forward, orig_tf, orig_ica
