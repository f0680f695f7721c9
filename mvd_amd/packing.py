"""State-dict (reference / diffusers key names) -> packed device weights for libmvd_hip.so.

One-time host work (torch is used as plumbing for the permutes / casts).  Slot layouts
(documented in DESIGN.md "Weight slots"):

  conv          [Cout][Cin/64][ky][kx][64] bf16  (K = 9*Cin; channel-slice major, taps inner)
  resnet conv2  conv2 | conv_shortcut(1x1) concatenated along K, biases summed
  attn1.qkv     [QSCALE*to_q; to_k; to_v; (QSCALE*to_q_ref)]   rows concatenated; QSCALE = 64^-0.5 * log2(e)
  attn1.out     [to_out.0 | ref_scale * to_out_ref.0]     K concatenated, bias = b + ref_scale*b_ref
  attn2.q       [QSCALE*to_q; (QSCALE*to_q_ref)]     text_kv: every attn2 site's [to_k; to_v] stacked in module order
  ref_kv        [to_k_ref(self); to_v_ref(self); to_k_ref(cross); to_v_ref(cross)]
  ff1           GEGLU rows interleaved in blocks of 16: (16 value rows, 16 gate rows)
  temb_proj     every resnet's time_emb_proj stacked in module order (one GEMM per forward)
  tail          [proj_out . ff.net.2 | proj_out]          K concatenated over [ff | h], bias = Wp.b2 + bp (compose_tail; replaces ff2 / proj_out)
  <slot>.wf/.cf LayerNorm-folded twins of attn1.qkv / attn2.q / ff1 (fold_layernorm): the fused LayerNorm GEMM reads the
                un-normalised rows; packed for C <= LN_FOLD_MAX_C (the levels whose GEMMs are big enough for that kernel)
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple


import torch

from .config import UNetConfig

# softmax scale of a 64-wide head times log2(e): folded into every query projection (see pack_unet)
QSCALE = 64 ** -0.5 * 1.4426950408889634


def _bf(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).to(torch.bfloat16).contiguous()


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _conv_w(w: torch.Tensor, tap_major: bool = False) -> torch.Tensor:
    """[Cout][Cin][3][3] -> [Cout][K].  Implicit-GEMM convs use K = [Cin/64][ky][kx][64] (channel-slice major: the
    nine taps of a 64-channel slice are consecutive K slabs -> L2-resident re-reads); conv_in / conv_out (and any
    Cin that is not a multiple of 64) use the plain tap-major [ky][kx][Cin]."""
    co, ci, kh, kw = w.shape
    w = w.detach().float()
    if tap_major or ci % 64:
        return w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
    return w.reshape(co, ci // 64, 64, kh, kw).permute(0, 1, 3, 4, 2).reshape(co, kh * kw * ci)


def block_weight(w: torch.Tensor) -> torch.Tensor:
    """[N][K] (K contiguous) -> the blocked layout of the small-M kernels (gemm_sm.hip, ``MvdGemmArgs::w_blocked``):
    [N/32][K/64] blocks of 32 rows x 128 bytes stored as the LDS image itself -- the 16-byte chunk ``c`` of row ``r`` sits in
    slot ``c ^ ((r >> 1) & 7)`` -- so that one LDS-DMA instruction of a workgroup copies one contiguous 4 KB block and a work
    item's K slice of a 32-row band is one contiguous range of HBM.  Same number of elements as ``w``."""
    n, k = w.shape
    assert n % 32 == 0 and k % 64 == 0, (n, k)
    b = w.reshape(n // 32, 32, k // 64, 8, 8).permute(0, 2, 1, 3, 4)            # [nb][kb][row][chunk][8]
    r = torch.arange(32, device=w.device)
    slot = torch.arange(8, device=w.device)
    src = slot[None, :] ^ ((r[:, None] >> 1) & 7)                               # chunk held by (row, slot)
    idx = src[None, None, :, :, None].expand(n // 32, k // 64, 32, 8, 8)
    return torch.gather(b, 3, idx).contiguous().reshape(n, k)


def _geglu_rows(w: torch.Tensor) -> torch.Tensor:
    """[8C, ...] -> rows re-ordered so each block of 32 = 16 value rows then the 16 matching gate rows."""
    half = w.shape[0] // 2
    val, gate = w[:half], w[half:]
    rest = w.shape[1:]
    v = val.reshape(half // 16, 1, 16, *rest)
    g = gate.reshape(half // 16, 1, 16, *rest)
    return torch.cat([v, g], dim=1).reshape(w.shape)


XS_K = 320      # operand width of the X-stationary kernels (gemm_xs.hip): the 64x64 level of SD-2.1


def _xs_row_perm(device) -> torch.Tensor:
    """MFMA row m of a 32-row unit -> channel of the unit it must hold so that lane (token, h) ends up with the 16
    CONSECUTIVE channels 16 h .. 16 h + 15 in its 16 accumulator registers (v_mfma_f32_32x32x16_bf16: register q of half h
    is row (q & 3) + 8 (q >> 2) + 4 h)."""
    m = torch.arange(32, device=device)
    return 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3)


def pack_xs(w: torch.Tensor, bias, geglu: bool = False, device=None) -> torch.Tensor:
    """[N][K] (+ bias [N] or None) -> the weight stream of gemm_xs.hip: ``[units][K/16 + 1][64][8]`` bf16.

    A unit is a 32-row tile in the order the kernel consumes it: k-step ``s < K/16`` is one MFMA A-operand fragment (lane
    ``(r, h)`` holds ``W[row(r)][16 s + 8 h .. + 8]``, rows permuted by ``_xs_row_perm``), the last k-step carries the bias
    split into two bf16 (hi at k = 0, lo at k = 1 of half 0) against the kernel's constant 1.0 operand.  ``geglu``: ``w``
    holds the value rows then the gate rows (diffusers' GEGLU.proj); units alternate gate | value of one 32-channel tile."""
    device = device if device is not None else w.device
    w = w.detach().to(device=device, dtype=torch.float32)
    n, k = w.shape
    assert k % 16 == 0 and n % (64 if geglu else 32) == 0, (n, k)
    b = torch.zeros(n, device=device) if bias is None else bias.detach().to(device=device, dtype=torch.float32)
    if geglu:
        half = n // 2
        order = torch.stack([torch.arange(half, n, device=device).reshape(-1, 32),          # gate tile j
                             torch.arange(0, half, device=device).reshape(-1, 32)], 1).reshape(-1)   # value tile j
        w, b = w[order], b[order]
    units, ks = n // 32, k // 16
    perm = _xs_row_perm(device)
    wu = w.reshape(units, 32, k)[:, perm]                                   # [unit][m][k]: MFMA row order
    bu = b.reshape(units, 32)[:, perm]
    frag = wu.reshape(units, 32, ks, 2, 8).permute(0, 2, 3, 1, 4)           # [unit][s][h][r][8]
    out = torch.zeros(units, ks + 1, 2, 32, 8, device=device, dtype=torch.bfloat16)
    out[:, :ks] = frag.to(torch.bfloat16)
    hi = bu.to(torch.bfloat16)
    lo = (bu - hi.float()).to(torch.bfloat16)
    out[:, ks, 0, :, 0] = hi
    out[:, ks, 0, :, 1] = lo
    return out.reshape(units, ks + 1, 64, 8).contiguous()


def pack_ws(w4: torch.Tensor, wsc=None, device=None) -> torch.Tensor:
    """conv weight ``[N][C][3][3]`` (+ 1x1 shortcut weight ``[N][Csc]`` or None) -> the weight stream of conv_ws.hip:
    per 16-channel column tile, the convolution's rounds ``[C/128][wave 4][tap 9][lane 64][8]`` then the shortcut's rounds
    ``[Csc/128][wave 4][lane 64][8]`` (bf16).  Lane ``(i, h) = (lane & 15, lane >> 4)`` of a 1 KB block holds the MFMA A-operand
    fragment ``W[16 ct + i][128 rd + 32 wave + 8 h .. + 8]`` of tap ``3 ky + kx`` (input pixel (y + ky - 1, x + kx - 1))."""
    device = device if device is not None else w4.device
    w4 = w4.detach().to(device=device, dtype=torch.float32)
    n, c = w4.shape[0], w4.shape[1]
    assert n % 16 == 0 and c % 128 == 0 and tuple(w4.shape[2:]) == (3, 3), tuple(w4.shape)
    t = w4.permute(0, 2, 3, 1).reshape(n // 16, 16, 9, c // 128, 4, 4, 8)        # [ct][i][tap][rd][wave][h][8]
    conv = t.permute(0, 3, 4, 2, 5, 1, 6).reshape(n // 16, -1)                   # [ct][rd][wave][tap][h][i][8]
    parts = [conv]
    if wsc is not None:
        wsc = wsc.detach().to(device=device, dtype=torch.float32).reshape(n, -1)
        sc = wsc.shape[1]
        assert sc % 128 == 0, sc
        u = wsc.reshape(n // 16, 16, sc // 128, 4, 4, 8)                         # [ct][i][rd][wave][h][8]
        parts.append(u.permute(0, 2, 3, 4, 1, 5).reshape(n // 16, -1))           # [ct][rd][wave][h][i][8]
    return torch.cat(parts, 1).to(torch.bfloat16).contiguous().reshape(-1)


def up4_weights(w: torch.Tensor) -> torch.Tensor:
    """3x3 weight ``[Cout][Cin][3][3]`` of a convolution behind a nearest-2x upsample -> the four 2x2 sub-pixel weights
    ``[parity py*2+px][Cout][Cin][ty][tx]`` (unrounded, fp32 or wider as ``w`` is).  In the upsampled map two of the three rows
    a window touches are the same source row, so output pixel (2i+py, 2j+px) is a 2x2 convolution of the SOURCE map whose
    window starts at (i+py-1, j+px-1): py = 0 weighs source rows (i-1, i) by (w[0], w[1]+w[2]), py = 1 weighs (i, i+1) by
    (w[0]+w[1], w[2]); the same along x.  Taps outside the source map are zero, as the padding of the upsampled map is."""
    assert w.dim() == 4 and tuple(w.shape[2:]) == (3, 3), tuple(w.shape)
    w = w.detach()
    if w.dtype not in (torch.float32, torch.float64):
        w = w.float()
    r = torch.tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=w.dtype, device=w.device)   # [parity][tap][k]
    w4 = torch.einsum("pty,qsx,oiyx->pqoits", r, r, w)                        # [py][px][Cout][Cin][ty][tx]
    return w4.reshape(4, w.shape[0], w.shape[1], 2, 2)


def pack_up4(w: torch.Tensor, device=None) -> torch.Tensor:
    """``[Cout][Cin][3][3]`` (the fp32 master) -> the ``.up.w4`` slot of the 2x2 sub-pixel upsampler (gemm_pp.hip, AMODE 4):
    ``[4 parities][Cout][K = 4*Cin]`` bf16, summed in fp32 and rounded once, K ordered like every conv slot of that kernel:
    ``[Cin/64][tap ty*2+tx][64]``."""
    device = device if device is not None else w.device
    w4 = up4_weights(w.detach().to(device=device, dtype=torch.float32))
    co, ci = w4.shape[1], w4.shape[2]
    assert ci % 64 == 0, ci
    k = w4.reshape(4, co, ci // 64, 64, 2, 2).permute(0, 1, 2, 4, 5, 3).reshape(4, co, 4 * ci)
    return k.to(torch.bfloat16).contiguous()


# LayerNorm fold: only the 64x64 / 32x32 levels (C = 320 / 640 in SD-2.1) ever reach the fused kernel (it needs >= 200
# tiles of 256x320, i.e. many rows); deeper levels keep ln_kernel + the plain GEMM and get no folded twin
LN_FOLD_MAX_C = 1 << 30     # every level: the small-M kernels (batch 1) fold at C = 1280 too (the M = 32-images kernels stop at 640)
LN_FOLD_LARGE_BATCH_MAX_C = 640   # what the many-images kernels (gemm_pp / gemm_xs: mvd_gemm_ln_fold_ok) ever read


def fold_layernorm(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias, device):
    """LayerNorm(x).W^T + b  ==  rstd*(x.Wf^T - mean*c1) + c2  with  Wf = W.diag(gamma) (bf16), c1 = Wf.1 (summed over the
    bf16 values, so that the mean term cancels exactly what the GEMM accumulated), c2 = W.beta + b.  Returns (wf, cf[2][N])."""
    w, gamma, beta = w.detach().float(), gamma.detach().float(), beta.detach().float()
    wf = (w * gamma[None, :]).to(torch.bfloat16)
    c1 = wf.float().sum(1)
    c2 = w @ beta
    if bias is not None:
        c2 = c2 + bias.detach().float()
    return wf.to(device).contiguous(), torch.stack([c1, c2], 0).to(device=device, dtype=torch.float32).contiguous()


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16 with ONE round-to-nearest-even.  torch converts through fp32, which rounds twice: a value that the fp32 step
    moves exactly onto the midpoint of two bf16 neighbours (the low half-word 0x8000) then goes to the even one, whichever side
    it came from.  Those elements -- about one in 2^16 -- take the neighbour on their own side instead."""
    assert t.dtype == torch.float64, t.dtype
    f = t.to(torch.float32)
    bits = f.contiguous().view(torch.int32)
    back = f.to(torch.float64)
    fix = ((bits & 0xFFFF) == 0x8000) & (back != t) & torch.isfinite(f)
    away = (t.abs() > back.abs()).to(torch.int32) << 16          # (sign-magnitude: + 0x10000 steps away from zero)
    fixed = (((bits >> 16) << 16) + away).view(torch.float32)   # an exact bf16 value: the conversion below keeps it
    return torch.where(fix, fixed, f).to(torch.bfloat16)


def compose_tail(w2: torch.Tensor, b2: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor):
    """ff.net.2 (``w2`` [C][4C], ``b2``) followed by proj_out (``wp`` [C][C], ``bp``) as ONE linear map over the two sources [ff | h]:

        h' = h + ff.W2^T + b2;  out = x + h'.Wp^T + bp   ==   out = x + [ff | h].[Wp.W2 | Wp]^T + (Wp.b2 + bp)

    composed on the host in fp64 from the master weights.  Returns (weight [C][5C] fp64 -- the caller rounds it to bf16 once, with
    ``round_bf16`` -- and bias [C] fp64)."""
    w2, b2, wp, bp = (t.detach().to(device="cpu", dtype=torch.float64) for t in (w2, b2, wp, bp))
    return torch.cat([wp @ w2, wp], dim=1), wp @ b2 + bp


def ws_twin_shapes_ok(c: int, n: int, scc0: int, scc1: int) -> bool:
    """The channel rules of conv_ws.hip ``mvd_conv_ws_applicable``: input width a multiple of 128 (a round), output width a multiple
    of 16 (a column tile), and EACH source of a fused 1x1 shortcut a multiple of 128 on its own (the halves of a skip
    concatenation are separate tensors)."""
    return c > 0 and c % 128 == 0 and n > 0 and n % 16 == 0 and scc0 % 128 == 0 and scc1 % 128 == 0 and not (scc1 and not scc0)


def pack_unet(sd: Dict[str, torch.Tensor], cfg: UNetConfig, device, adapter: bool, ref_scale: float = 0.0,
              small_batch_twins: bool = True, fold_tail: bool = True) -> Dict[str, torch.Tensor]:
    """``sd`` holds diffusers keys (no wrapper prefix) and, when ``adapter``, the ``...processor.*`` keys.

    ``fold_tail`` (the default): every transformer site gets ``<key>.tail.w`` / ``.tail.b`` -- ff.net.2 and proj_out composed into one
    K-concatenated GEMM (``compose_tail``) -- INSTEAD of ``ff2.w/.b`` and ``proj_out.w/.b/.wx``: the same number of weight elements,
    one launch less per site.  ``fold_tail=False`` packs the five old slots and the engine runs the two launches (the A/B switch:
    the engine picks the route by which slots are registered).

    ``small_batch_twins=False`` leaves out the second copies only a batch-1 forward reads -- the weight-streaming ``.ws``
    convolution twins (conv_ws.hip) and the LayerNorm-folded ``.wf/.cf`` twins above C = 640 (gemm_sm.hip): ~1.4 GB per SD-2.1
    weight set.  The engine looks every twin up by name and takes the tiled convolution / ln_kernel + plain GEMM route when it is
    absent (engine.hip ``try_ws`` / ``ln_gemm``), so a deployment that only ever runs many-image batches loses nothing."""
    fold_max_c = LN_FOLD_MAX_C if small_batch_twins else LN_FOLD_LARGE_BATCH_MAX_C
    out: Dict[str, torch.Tensor] = {}
    w_in = _conv_w(sd["conv_in.weight"], tap_major=True)                       # [C0][9*Cin] -> zero padded to K = 64 (one MFMA slab)
    out["conv_in.w"] = _bf(torch.nn.functional.pad(w_in, (0, 64 - w_in.shape[1])), device)
    out["conv_in.b"] = _f32(sd["conv_in.bias"], device)
    out["time.l1.w"] = _bf(sd["time_embedding.linear_1.weight"], device)
    out["time.l1.b"] = _f32(sd["time_embedding.linear_1.bias"], device)
    out["time.l2.w"] = _bf(sd["time_embedding.linear_2.weight"], device)
    out["time.l2.b"] = _f32(sd["time_embedding.linear_2.bias"], device)
    tw, tb = [], []
    split = cfg.resnet_input_split()
    for key, cin, cout in cfg.resnets():
        out[f"{key}.norm1.g"] = _f32(sd[f"{key}.norm1.weight"], device)
        out[f"{key}.norm1.b"] = _f32(sd[f"{key}.norm1.bias"], device)
        out[f"{key}.conv1.w"] = _bf(_conv_w(sd[f"{key}.conv1.weight"]), device)
        out[f"{key}.conv1.b"] = _f32(sd[f"{key}.conv1.bias"], device)
        out[f"{key}.norm2.g"] = _f32(sd[f"{key}.norm2.weight"], device)
        out[f"{key}.norm2.b"] = _f32(sd[f"{key}.norm2.bias"], device)
        w2 = _conv_w(sd[f"{key}.conv2.weight"])
        b2 = sd[f"{key}.conv2.bias"].detach().float()
        if cin != cout:
            w2 = torch.cat([w2, sd[f"{key}.conv_shortcut.weight"].detach().float().reshape(cout, cin)], dim=1)
            b2 = b2 + sd[f"{key}.conv_shortcut.bias"].detach().float()
        out[f"{key}.conv2.w"] = _bf(w2, device)
        out[f"{key}.conv2.b"] = _f32(b2, device)
        # weight-streaming twins (conv_ws.hip) for every level but the first -- the 32x32, 16x16 and 8x8 maps of a 64x64 latent,
        # where a batch-1 launch is a weight stream -- and only where the kernel's shape predicate can ever say yes
        # (ws_twin_shapes_ok = mvd_conv_ws_applicable's channel rules: a twin nothing can read is not packed, nor broadcast)
        if small_batch_twins and cout > cfg.block_out_channels[0]:
            if ws_twin_shapes_ok(cin, cout, 0, 0):
                out[f"{key}.conv1.ws"] = pack_ws(sd[f"{key}.conv1.weight"], None, device)
            if cin == cout:
                if ws_twin_shapes_ok(cout, cout, 0, 0):
                    out[f"{key}.conv2.ws"] = pack_ws(sd[f"{key}.conv2.weight"], None, device)
            elif ws_twin_shapes_ok(cout, cout, *split[key]):
                out[f"{key}.conv2.ws"] = pack_ws(sd[f"{key}.conv2.weight"], sd[f"{key}.conv_shortcut.weight"].reshape(cout, cin), device)
        tw.append(sd[f"{key}.time_emb_proj.weight"].detach().float())
        tb.append(sd[f"{key}.time_emb_proj.bias"].detach().float())
    out["temb_proj.w"] = _bf(torch.cat(tw, 0), device)
    out["temb_proj.b"] = _f32(torch.cat(tb, 0), device)

    tkv = []   # text K/V projections of every attn2 site, stacked in module order (one GEMM per pass)
    for key, _feat, C, _heads in cfg.transformers():
        b = f"{key}.transformer_blocks.0"
        out[f"{key}.norm.g"] = _f32(sd[f"{key}.norm.weight"], device)
        out[f"{key}.norm.b"] = _f32(sd[f"{key}.norm.bias"], device)
        out[f"{key}.proj_in.w"] = _bf(sd[f"{key}.proj_in.weight"], device)
        out[f"{key}.proj_in.b"] = _f32(sd[f"{key}.proj_in.bias"], device)
        if fold_tail:
            wt, bt = compose_tail(sd[f"{b}.ff.net.2.weight"], sd[f"{b}.ff.net.2.bias"], sd[f"{key}.proj_out.weight"], sd[f"{key}.proj_out.bias"])
            out[f"{key}.tail.w"] = round_bf16(wt).to(device).contiguous()
            out[f"{key}.tail.b"] = _f32(bt, device)
        else:
            out[f"{key}.proj_out.w"] = _bf(sd[f"{key}.proj_out.weight"], device)
            out[f"{key}.proj_out.b"] = _f32(sd[f"{key}.proj_out.bias"], device)
            out[f"{key}.ff2.w"] = _bf(sd[f"{b}.ff.net.2.weight"], device)
            out[f"{key}.ff2.b"] = _f32(sd[f"{b}.ff.net.2.bias"], device)
        for i in (1, 2, 3):
            out[f"{key}.ln{i}.g"] = _f32(sd[f"{b}.norm{i}.weight"], device)
            out[f"{key}.ln{i}.b"] = _f32(sd[f"{b}.norm{i}.bias"], device)
        f = lambda k: sd[k].detach().float()  # noqa: E731
        # every query projection carries the softmax scale and log2(e): the attention kernel then works in the exp2
        # domain without a per-score multiply (attn_kernel<.., PRE>); the factor is applied in fp32 before the bf16
        # rounding of the weights
        qkv = [QSCALE * f(f"{b}.attn1.to_q.weight"), f(f"{b}.attn1.to_k.weight"), f(f"{b}.attn1.to_v.weight")]
        q2 = [QSCALE * f(f"{b}.attn2.to_q.weight")]
        for a in ("attn1", "attn2"):
            wo, bo = f(f"{b}.{a}.to_out.0.weight"), f(f"{b}.{a}.to_out.0.bias")
            if adapter:
                pr = f"{b}.{a}.processor"
                out[f"{key}.{a}.out.b0"] = _f32(bo, device)      # plain bias for passes without the adapter
                wo = torch.cat([wo, ref_scale * f(f"{pr}.to_out_ref.0.weight")], dim=1)
                bo = bo + ref_scale * f(f"{pr}.to_out_ref.0.bias")
            out[f"{key}.{a}.out.w"] = _bf(wo, device)
            out[f"{key}.{a}.out.b"] = _f32(bo, device)
        if adapter:
            p1, p2 = f"{b}.attn1.processor", f"{b}.attn2.processor"
            qkv.append(QSCALE * f(f"{p1}.to_q_ref.weight"))
            q2.append(QSCALE * f(f"{p2}.to_q_ref.weight"))
            out[f"{key}.ref_kv.w"] = _bf(torch.cat([f(f"{p1}.to_k_ref.weight"), f(f"{p1}.to_v_ref.weight"),
                                                    f(f"{p2}.to_k_ref.weight"), f(f"{p2}.to_v_ref.weight")], 0), device)
        out[f"{key}.attn1.qkv.w"] = _bf(torch.cat(qkv, 0), device)
        out[f"{key}.attn2.q.w"] = _bf(torch.cat(q2, 0), device)
        tkv.append(torch.cat([f(f"{b}.attn2.to_k.weight"), f(f"{b}.attn2.to_v.weight")], 0))
        ff1_w, ff1_b = _geglu_rows(f(f"{b}.ff.net.0.proj.weight")), _geglu_rows(f(f"{b}.ff.net.0.proj.bias"))
        out[f"{key}.ff1.w"] = _bf(ff1_w, device)
        out[f"{key}.ff1.b"] = _f32(ff1_b, device)
        if C <= fold_max_c:
            for slot, w, bias, i in ((f"{key}.attn1.qkv", torch.cat(qkv, 0), None, 1), (f"{key}.attn2.q", torch.cat(q2, 0), None, 2),
                                     (f"{key}.ff1", ff1_w, ff1_b, 3)):
                out[f"{slot}.wf"], out[f"{slot}.cf"] = fold_layernorm(w, f(f"{b}.norm{i}.weight"), f(f"{b}.norm{i}.bias"), bias, device)
        if C == XS_K:
            # twins for the X-stationary kernels (gemm_xs.hip): the K = 320 projections of the 64x64 level
            out[f"{key}.proj_in.wx"] = pack_xs(f(f"{key}.proj_in.weight"), f(f"{key}.proj_in.bias"), device=device)
            if not fold_tail:
                out[f"{key}.proj_out.wx"] = pack_xs(f(f"{key}.proj_out.weight"), f(f"{key}.proj_out.bias"), device=device)
            for a in ("attn1", "attn2"):   # the out-projection of a pass WITHOUT the adapter branch (K = C)
                out[f"{key}.{a}.out.wx"] = pack_xs(f(f"{b}.{a}.to_out.0.weight"), f(f"{b}.{a}.to_out.0.bias"), device=device)
            if adapter:
                out[f"{key}.ref_kv.wx"] = pack_xs(out[f"{key}.ref_kv.w"].float(), None, device=device)
            for slot, geglu in ((f"{key}.attn1.qkv", False), (f"{key}.attn2.q", False), (f"{key}.ff1", True)):
                wf, cf = out[f"{slot}.wf"].float(), out[f"{slot}.cf"]
                if geglu:    # .wf / .cf are in the 16 | 16 interleaved row order of the ping-pong kernel: undo it
                    inv = torch.argsort(_geglu_rows(torch.arange(wf.shape[0], device=wf.device)))
                    wf, cf = wf[inv], cf[:, inv]
                out[f"{slot}.wx"] = pack_xs(wf, cf[1], geglu=geglu, device=device)

    out["text_kv.w"] = _bf(torch.cat(tkv, 0), device)
    n = cfg.num_levels
    for i in range(n - 1):
        out[f"down_blocks.{i}.down.w"] = _bf(_conv_w(sd[f"down_blocks.{i}.downsamplers.0.conv.weight"]), device)
        out[f"down_blocks.{i}.down.b"] = _f32(sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], device)
        out[f"up_blocks.{i}.up.w"] = _bf(_conv_w(sd[f"up_blocks.{i}.upsamplers.0.conv.weight"]), device)
        wu = sd[f"up_blocks.{i}.upsamplers.0.conv.weight"]
        if small_batch_twins and wu.shape[0] > cfg.block_out_channels[0] and wu.shape[0] % 128 == 0 and wu.shape[1] % 128 == 0:
            out[f"up_blocks.{i}.up.ws"] = pack_ws(wu, None, device)            # conv_ws.hip with the 2x upsampling in front
        if wu.shape[1] % 64 == 0:
            out[f"up_blocks.{i}.up.w4"] = pack_up4(wu, device)                 # many-image batches: four 2x2 sub-pixel convolutions
        out[f"up_blocks.{i}.up.b"] = _f32(sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], device)
    out["conv_norm_out.g"] = _f32(sd["conv_norm_out.weight"], device)
    out["conv_norm_out.b"] = _f32(sd["conv_norm_out.bias"], device)
    out["conv_out.w"] = _bf(_conv_w(sd["conv_out.weight"], tap_major=True), device)
    out["conv_out.b"] = _f32(sd["conv_out.bias"], device)
    return out


def pack_camera(sd: Dict[str, torch.Tensor], device, num_levels: int = 4) -> Dict[str, torch.Tensor]:
    """Camera encoder stays fp32 (Q9): slots are the reference keys prefixed with ``cam.``.  In addition the modulator MLPs the
    hooks address (down_i, up_i, output -- the engine's order; ``mid`` is never addressed, Q3) are stored CONCATENATED
    (``cam.modcat.*``), so that all of them run as four launches instead of four each (the camera path is ~50 tiny launches
    in front of a batch-1 forward)."""
    out = {f"cam.{k}": _f32(v, device) for k, v in sd.items()}
    names = [f"down_{i}" for i in range(num_levels)] + [f"up_{i}" for i in range(num_levels)] + ["output"]
    keys = [f"modulators.{n}.{j}.{t}" for n in names for j in (0, 1, 3) for t in ("weight", "bias")]
    if all(k in sd for k in keys):
        cat = lambda j, t: torch.cat([sd[f"modulators.{n}.{j}.{t}"].detach().float() for n in names], 0)   # noqa: E731
        out["cam.modcat.w0"], out["cam.modcat.b0"] = _f32(cat(0, "weight"), device), _f32(cat(0, "bias"), device)
        out["cam.modcat.g1"], out["cam.modcat.be1"] = _f32(cat(1, "weight"), device), _f32(cat(1, "bias"), device)
        out["cam.modcat.w3"], out["cam.modcat.b3"] = _f32(cat(3, "weight"), device), _f32(cat(3, "bias"), device)
    return out


# ---------------------------------------------------------------------------------------------- VGG-16 (perceptual loss, row N8)
# torchvision's vgg16().features[:29]: (index, cin, cout) of the thirteen 3x3 pad-1 convolutions; a ReLU follows every one but
# the last (features.28), a 2x2 max-pool sits at VGG16_POOLS (behind relu1_2, relu2_2, relu3_3, relu4_3)
VGG16_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
               (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
VGG16_POOLS = (4, 9, 16, 23)
VGG16_PARAMS = 14_714_688          # over the 26 tensors


def normalize_vgg_keys(sd) -> Dict[str, torch.Tensor]:
    """A torchvision ``vgg16`` state dict (``features.N.*``; ``classifier.*`` and anything else is ignored) or the one of the
    sliced ``Sequential`` (``N.*``) -> the 26 tensors as ``features.N.weight`` / ``features.N.bias``.  A missing key or a wrong
    shape raises ``MvdError``."""
    from ._lib import MvdError
    if not hasattr(sd, "keys"):
        raise MvdError(f"VGG-16 weights: expected a state dict, got {type(sd).__name__}")
    out = {}
    for idx, cin, cout in VGG16_CONVS:
        for leaf, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            t = sd.get(f"features.{idx}.{leaf}", sd.get(f"{idx}.{leaf}"))
            if t is None:
                raise MvdError(f"VGG-16 weights: key 'features.{idx}.{leaf}' (or '{idx}.{leaf}') is missing")
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise MvdError(f"VGG-16 weights: 'features.{idx}.{leaf}' has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
            out[f"features.{idx}.{leaf}"] = t
    return out


def pack_vgg_conv(w: torch.Tensor) -> torch.Tensor:
    """[cout][cin][3][3] -> the packed fp32 [cout][K] of one tower convolution: the implicit-GEMM layout [cin/64][ky][kx][64] of
    ``_conv_w``, or for conv1_1 (cin = 3) the im2col order of ``im2col_in_kernel``, column tap * 3 + channel, zero padded 27 -> 64."""
    if w.shape[1] == 3:
        return torch.nn.functional.pad(_conv_w(w, tap_major=True), (0, 64 - 27))
    return _conv_w(w)


def pack_vgg(sd: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """``mvd_vgg_set_weight`` slots: ``features.N.weight`` bf16 (``pack_vgg_conv``), ``features.N.bias`` fp32."""
    sd = normalize_vgg_keys(sd)
    out = {}
    for idx, _, _ in VGG16_CONVS:
        out[f"features.{idx}.weight"] = _bf(pack_vgg_conv(sd[f"features.{idx}.weight"]), device)
        out[f"features.{idx}.bias"] = _f32(sd[f"features.{idx}.bias"], device)
    return out


# ---------------------------------------------------------------------------------------------- LPIPS (AlexNet / VGG-16 backbones, row N9)
# torchvision's alexnet().features[:12]: (index, cin, cout, kernel, stride, padding) of the five convolutions; a ReLU follows
# every one (the five LPIPS taps, at index + 1), a 3x3 stride-2 max-pool sits at ALEX_POOLS
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
ALEX_POOLS = (2, 5)
ALEX_TAP_CHANNELS = (64, 192, 384, 256, 256)
ALEX_CONV1_COLS = 384              # 11 * 11 * 3 = 363 columns of the im2col rows, zero padded to a multiple of 64
# the taps of the VGG variant: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of vgg16().features[:30]
VGG_LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def normalize_backbone_keys(sd, convs, what: str) -> Dict[str, torch.Tensor]:
    """The convolutions ``convs`` ((index, cin, cout, kernel, ...) or (index, cin, cout) with kernel 3) out of a state dict under
    torchvision's keys (``features.N.*``), those of the sliced ``Sequential`` (``N.*``) or lpips' (``net.sliceK.N.*``; a full
    ``lpips.LPIPS`` state dict carries them beside the linear heads) -> ``features.N.weight`` / ``features.N.bias``.  A missing key
    or a wrong shape raises ``MvdError``."""
    import re
    from ._lib import MvdError
    if not hasattr(sd, "keys"):
        raise MvdError(f"{what} weights: expected a state dict, got {type(sd).__name__}")
    found = {}
    for key in sd.keys():
        m = re.match(r"^(?:features\.|net\.slice\d+\.)?(\d+)\.(weight|bias)$", key)
        if m:
            found[(int(m.group(1)), m.group(2))] = sd[key]
    out = {}
    for conv in convs:
        idx, cin, cout = conv[:3]
        k = conv[3] if len(conv) > 3 else 3
        for leaf, shape in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            t = found.get((idx, leaf))
            if t is None:
                raise MvdError(f"{what} weights: key 'features.{idx}.{leaf}' (or '{idx}.{leaf}', 'net.sliceK.{idx}.{leaf}') is missing")
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise MvdError(f"{what} weights: 'features.{idx}.{leaf}' has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
            out[f"features.{idx}.{leaf}"] = t
    return out


def normalize_lpips_lin_keys(sd, channels, what: str = "LPIPS") -> Dict[str, torch.Tensor]:
    """lpips' linear heads (``lin{k}.model.1.weight`` or ``lins.{k}.model.1.weight``, shape (1, C, 1, 1)) -> ``lin{k}.weight`` fp32
    (C,).  A negative weight raises ``MvdError``: the shipped heads have none, and the head kernel's contract is w >= 0."""
    from ._lib import MvdError
    if not hasattr(sd, "keys"):
        raise MvdError(f"{what} linear heads: expected a state dict, got {type(sd).__name__}")
    out = {}
    for k, c in enumerate(channels):
        t = sd.get(f"lin{k}.model.1.weight", sd.get(f"lins.{k}.model.1.weight"))
        if t is None:
            raise MvdError(f"{what} linear heads: key 'lin{k}.model.1.weight' (or 'lins.{k}.model.1.weight') is missing")
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (1, c, 1, 1):
            raise MvdError(f"{what} linear heads: 'lin{k}.model.1.weight' has shape {tuple(getattr(t, 'shape', ()))}, expected {(1, c, 1, 1)}")
        t = t.detach().float().reshape(c)
        if bool((t < 0).any()):
            raise MvdError(f"{what} linear heads: 'lin{k}.model.1.weight' has a negative weight ({float(t.min()):.3e}); the head takes w >= 0 only")
        out[f"lin{k}.weight"] = t
    return out


def pack_alex_conv(w: torch.Tensor) -> torch.Tensor:
    """[cout][cin][k][k] -> the packed fp32 [cout][K] of one AlexNet convolution: conv1 (11x11) and conv2 (5x5) in the im2col
    order of ``im2col_patch_*_kernel``, column (ky * k + kx) * cin + c (conv1 zero padded 363 -> 384); the 3x3 ones in the
    implicit-GEMM layout [cin/64][ky][kx][64] of ``_conv_w``."""
    if w.shape[2] == 3:
        return _conv_w(w)
    flat = w.detach().float().permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return torch.nn.functional.pad(flat, (0, -flat.shape[1] % 64))


def pack_alex(backbone: Dict[str, torch.Tensor], lins: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """``mvd_lpips_set_weight`` slots: ``features.N.weight`` bf16 (``pack_alex_conv``), ``features.N.bias`` fp32, ``lin{k}.weight`` fp32"""
    sd = normalize_backbone_keys(backbone, ALEX_CONVS, "AlexNet")
    out = {}
    for conv in ALEX_CONVS:
        idx = conv[0]
        out[f"features.{idx}.weight"] = _bf(pack_alex_conv(sd[f"features.{idx}.weight"]), device)
        out[f"features.{idx}.bias"] = _f32(sd[f"features.{idx}.bias"], device)
    for k in range(5):
        out[f"lin{k}.weight"] = _f32(lins[f"lin{k}.weight"], device)
    return out


# ---------------------------------------------------------------------------------------------- FID: Inception-v3 up to pool3 (row N10)
# The FID variant of Inception-v3 (torch-fidelity's FeatureExtractorInceptionV3 / pytorch-fid's pt_inception-2015-12-05) as ONE
# table that the schedule (``fid_program`` -> mvd_fid_create), the packer (``pack_inception_fid``) and the tests' restatement
# (tests/fid_ref.py) all read.  Entries, in execution order:
#   ("conv", name, src, dst, c_off, cin, cout, kh, kw, stride, pad_h, pad_w)   BasicConv2d ``name``: conv (no bias) + BN(eps 1e-3) + ReLU
#   ("pool", mode, src, dst, c_off, c)                                         3x3 pool: "avg" (stride 1, pad 1, count_include_pad=False),
#                                                                              "max1" (stride 1, pad 1), "max2" (stride 2, no padding)
# ``src`` is read whole; the result goes to channels [c_off, c_off + cout) of ``dst`` -- a block's output buffer is its
# concatenation, in torch-fidelity's branch order.  "img" is the front end's output, FID_FEATURE_BUFFER the map pool3 averages.
FID_INPUT_SIZE = 299
FID_INPUT_CHANNELS = 16            # the front end writes r, g, b and 13 zero channels: the convolution reads multiples of 16
FID_BN_EPS = 1e-3
FID_FEATURE_BUFFER = "Mixed_7c"
FID_POOL_MODES = {"avg": 0, "max1": 1, "max2": 2}


def _inception_fid_layers():
    T = []

    def conv(name, src, dst, c_off, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
        T.append(("conv", name, src, dst, c_off, cin, cout, k[0], k[1], stride, pad[0], pad[1]))

    def pool(mode, src, dst, c_off, c):
        T.append(("pool", mode, src, dst, c_off, c))

    conv("Conv2d_1a_3x3", "img", "Conv2d_1a", 0, 3, 32, (3, 3), 2)
    conv("Conv2d_2a_3x3", "Conv2d_1a", "Conv2d_2a", 0, 32, 32, (3, 3))
    conv("Conv2d_2b_3x3", "Conv2d_2a", "Conv2d_2b", 0, 32, 64, (3, 3), 1, (1, 1))
    pool("max2", "Conv2d_2b", "MaxPool_1", 0, 64)
    conv("Conv2d_3b_1x1", "MaxPool_1", "Conv2d_3b", 0, 64, 80)
    conv("Conv2d_4a_3x3", "Conv2d_3b", "Conv2d_4a", 0, 80, 192, (3, 3))
    pool("max2", "Conv2d_4a", "MaxPool_2", 0, 192)
    x = "MaxPool_2"
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):                 # A
        conv(f"{blk}.branch1x1", x, blk, 0, cin, 64)
        conv(f"{blk}.branch5x5_1", x, f"{blk}.t5", 0, cin, 48)
        conv(f"{blk}.branch5x5_2", f"{blk}.t5", blk, 64, 48, 64, (5, 5), 1, (2, 2))
        conv(f"{blk}.branch3x3dbl_1", x, f"{blk}.t3a", 0, cin, 64)
        conv(f"{blk}.branch3x3dbl_2", f"{blk}.t3a", f"{blk}.t3b", 0, 64, 96, (3, 3), 1, (1, 1))
        conv(f"{blk}.branch3x3dbl_3", f"{blk}.t3b", blk, 128, 96, 96, (3, 3), 1, (1, 1))
        pool("avg", x, f"{blk}.tp", 0, cin)
        conv(f"{blk}.branch_pool", f"{blk}.tp", blk, 224, cin, pf)
        x = blk
    blk = "Mixed_6a"                                                                                            # B
    conv(f"{blk}.branch3x3", x, blk, 0, 288, 384, (3, 3), 2)
    conv(f"{blk}.branch3x3dbl_1", x, f"{blk}.t3a", 0, 288, 64)
    conv(f"{blk}.branch3x3dbl_2", f"{blk}.t3a", f"{blk}.t3b", 0, 64, 96, (3, 3), 1, (1, 1))
    conv(f"{blk}.branch3x3dbl_3", f"{blk}.t3b", blk, 384, 96, 96, (3, 3), 2)
    pool("max2", x, blk, 480, 288)
    x = blk
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):                # C
        conv(f"{blk}.branch1x1", x, blk, 0, 768, 192)
        conv(f"{blk}.branch7x7_1", x, f"{blk}.t7a", 0, 768, c7)
        conv(f"{blk}.branch7x7_2", f"{blk}.t7a", f"{blk}.t7b", 0, c7, c7, (1, 7), 1, (0, 3))
        conv(f"{blk}.branch7x7_3", f"{blk}.t7b", blk, 192, c7, 192, (7, 1), 1, (3, 0))
        conv(f"{blk}.branch7x7dbl_1", x, f"{blk}.d1", 0, 768, c7)
        conv(f"{blk}.branch7x7dbl_2", f"{blk}.d1", f"{blk}.d2", 0, c7, c7, (7, 1), 1, (3, 0))
        conv(f"{blk}.branch7x7dbl_3", f"{blk}.d2", f"{blk}.d3", 0, c7, c7, (1, 7), 1, (0, 3))
        conv(f"{blk}.branch7x7dbl_4", f"{blk}.d3", f"{blk}.d4", 0, c7, c7, (7, 1), 1, (3, 0))
        conv(f"{blk}.branch7x7dbl_5", f"{blk}.d4", blk, 384, c7, 192, (1, 7), 1, (0, 3))
        pool("avg", x, f"{blk}.tp", 0, 768)
        conv(f"{blk}.branch_pool", f"{blk}.tp", blk, 576, 768, 192)
        x = blk
    blk = "Mixed_7a"                                                                                            # D
    conv(f"{blk}.branch3x3_1", x, f"{blk}.t3", 0, 768, 192)
    conv(f"{blk}.branch3x3_2", f"{blk}.t3", blk, 0, 192, 320, (3, 3), 2)
    conv(f"{blk}.branch7x7x3_1", x, f"{blk}.s1", 0, 768, 192)
    conv(f"{blk}.branch7x7x3_2", f"{blk}.s1", f"{blk}.s2", 0, 192, 192, (1, 7), 1, (0, 3))
    conv(f"{blk}.branch7x7x3_3", f"{blk}.s2", f"{blk}.s3", 0, 192, 192, (7, 1), 1, (3, 0))
    conv(f"{blk}.branch7x7x3_4", f"{blk}.s3", blk, 320, 192, 192, (3, 3), 2)
    pool("max2", x, blk, 512, 768)
    x = blk
    for blk, cin, mode in (("Mixed_7b", 1280, "avg"), ("Mixed_7c", 2048, "max1")):                              # E
        conv(f"{blk}.branch1x1", x, blk, 0, cin, 320)
        conv(f"{blk}.branch3x3_1", x, f"{blk}.t3", 0, cin, 384)
        conv(f"{blk}.branch3x3_2a", f"{blk}.t3", blk, 320, 384, 384, (1, 3), 1, (0, 1))
        conv(f"{blk}.branch3x3_2b", f"{blk}.t3", blk, 704, 384, 384, (3, 1), 1, (1, 0))
        conv(f"{blk}.branch3x3dbl_1", x, f"{blk}.d1", 0, cin, 448)
        conv(f"{blk}.branch3x3dbl_2", f"{blk}.d1", f"{blk}.d2", 0, 448, 384, (3, 3), 1, (1, 1))
        conv(f"{blk}.branch3x3dbl_3a", f"{blk}.d2", blk, 1088, 384, 384, (1, 3), 1, (0, 1))
        conv(f"{blk}.branch3x3dbl_3b", f"{blk}.d2", blk, 1472, 384, 384, (3, 1), 1, (1, 0))
        pool(mode, x, f"{blk}.tp", 0, cin)
        conv(f"{blk}.branch_pool", f"{blk}.tp", blk, 1856, cin, 192)
        x = blk
    return tuple(T)


INCEPTION_FID_LAYERS = _inception_fid_layers()
INCEPTION_FID_CONVS = tuple(e for e in INCEPTION_FID_LAYERS if e[0] == "conv")


def fid_buffer_channels(layers=INCEPTION_FID_LAYERS) -> Dict[str, int]:
    """logical channels of every buffer of the table: the widest slice anything writes ("img": 3)"""
    ch = {"img": 3}
    for e in layers:
        dst, end = e[3], e[4] + (e[6] if e[0] == "conv" else e[5])
        ch[dst] = max(ch.get(dst, 0), end)
    return ch


def fid_geometry(layers=INCEPTION_FID_LAYERS, size: int = FID_INPUT_SIZE) -> Dict[str, Tuple[int, int]]:
    """(h, w) of every buffer for a ``size`` x ``size`` input"""
    hw = {"img": (size, size)}
    for e in layers:
        h, w = hw[e[2]]
        if e[0] == "conv":
            _, _, _, dst, _, _, _, kh, kw, s, ph, pw = e
            o = ((h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1)
        else:
            dst = e[3]
            o = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if e[1] == "max2" else (h, w)
        assert hw.setdefault(dst, o) == o, f"{dst}: {hw[dst]} and {o}"
    return hw


def fid_parameter_count(layers=INCEPTION_FID_LAYERS) -> int:
    """convolution weights plus the four BatchNorm vectors of every BasicConv2d of the table"""
    return sum(e[6] * e[5] * e[7] * e[8] + 4 * e[6] for e in layers if e[0] == "conv")


def fid_program(layers=INCEPTION_FID_LAYERS):
    """The table compiled for ``mvd_fid_create``: (program ints, 13 per entry; buffer ints, (channels, is_fp32) per buffer; the
    convolutions' names; the index of the feature buffer).  Buffer 0 is "img" with its ``FID_INPUT_CHANNELS`` physical channels;
    the feature buffer alone is fp32."""
    ch = fid_buffer_channels(layers)
    ch["img"] = FID_INPUT_CHANNELS
    ids = {name: i for i, name in enumerate(ch)}
    prog, names = [], []
    for e in layers:
        if e[0] == "conv":
            _, name, src, dst, c_off, cin, cout, kh, kw, s, ph, pw = e
            prog += [0, ids[src], ids[dst], c_off, ch[src], cout, kh, kw, s, ph, pw, len(names), 0]
            names.append(name)
        else:
            _, mode, src, dst, c_off, c = e
            prog += [1, ids[src], ids[dst], c_off, c, c, 3, 3, 2 if mode == "max2" else 1, 0 if mode == "max2" else 1, 0 if mode == "max2" else 1, -1,
                     FID_POOL_MODES[mode]]
    bufs = []
    for name, c in ch.items():
        bufs += [c, int(name == FID_FEATURE_BUFFER)]
    return prog, bufs, names, ids[FID_FEATURE_BUFFER]


def fold_batchnorm(w: torch.Tensor, gamma, beta, mean, var, eps: float = FID_BN_EPS):
    """conv (no bias) + BatchNorm (eval) as one convolution, in fp32: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)"""
    s = gamma.detach().float() / torch.sqrt(var.detach().float() + eps)
    return w.detach().float() * s.view(-1, 1, 1, 1), beta.detach().float() - mean.detach().float() * s


def fid_cin_pad(cin: int) -> int:
    return (cin + 31) // 32 * 32


def pack_slice_conv(w: torch.Tensor, cin_phys: int = 0) -> torch.Tensor:
    """[cout][cin][kh][kw] -> [cout][kh kw cin_pad] of ``mvd_op_conv_relu_slice``: column (ky kw + kx) cin_pad + c with cin_pad =
    max(cin, cin_phys) rounded up to 32 and zeros in the padding (dtype kept)."""
    cout, cin, kh, kw = w.shape
    pad = fid_cin_pad(max(cin, cin_phys))
    t = torch.nn.functional.pad(w.detach().permute(0, 2, 3, 1), (0, pad - cin))
    return t.reshape(cout, kh * kw * pad).contiguous()


def normalize_inception_fid_keys(sd) -> Dict[str, torch.Tensor]:
    """torch-fidelity's / pytorch-fid's state dict -> the five tensors of every BasicConv2d of the table under
    ``<name>.conv.weight`` / ``<name>.bn.{weight,bias,running_mean,running_var}``; ``fc.*``, ``num_batches_tracked`` and anything
    else is ignored, a ``module.`` / ``model.`` / ``inception.`` prefix dropped.  A missing key or a wrong shape raises ``MvdError``."""
    from ._lib import MvdError
    if not hasattr(sd, "keys"):
        raise MvdError(f"Inception-v3 (FID) weights: expected a state dict, got {type(sd).__name__}")
    found = {}
    for key in sd.keys():
        k = key
        for prefix in ("module.", "model.", "inception.", "base."):
            if k.startswith(prefix):
                k = k[len(prefix):]
        found[k] = sd[key]
    out = {}
    for e in INCEPTION_FID_CONVS:
        name, cin, cout, kh, kw = e[1], e[5], e[6], e[7], e[8]
        for leaf, shape in (("conv.weight", (cout, cin, kh, kw)), ("bn.weight", (cout,)), ("bn.bias", (cout,)), ("bn.running_mean", (cout,)),
                            ("bn.running_var", (cout,))):
            t = found.get(f"{name}.{leaf}")
            if t is None:
                raise MvdError(f"Inception-v3 (FID) weights: key '{name}.{leaf}' is missing")
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise MvdError(f"Inception-v3 (FID) weights: '{name}.{leaf}' has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
            out[f"{name}.{leaf}"] = t
    return out


INCEPTION_FC_SHAPE = (1008, 2048)      # torch-fidelity's fc of the FID Inception-v3: 1008 classes over pool3


def inception_fc_weight(sd, required: bool = True) -> Optional[torch.Tensor]:
    """``fc.weight`` (1008, 2048) of a torch-fidelity / pytorch-fid state dict as contiguous fp32, under the prefixes
    ``normalize_inception_fid_keys`` strips; ``fc.bias`` is not used (``logits_unbiased``).  Without the key: ``MvdError``, or
    ``None`` when not ``required``; a wrong shape always raises."""
    from ._lib import MvdError
    if not hasattr(sd, "keys"):
        raise MvdError(f"Inception-v3 (FID) weights: expected a state dict, got {type(sd).__name__}")
    t = None
    for key in sd.keys():
        k = key
        for prefix in ("module.", "model.", "inception.", "base."):
            if k.startswith(prefix):
                k = k[len(prefix):]
        if k == "fc.weight":
            t = sd[key]
            break
    if t is None:
        if required:
            raise MvdError("Inception-v3 (FID) weights: key 'fc.weight' is missing (the Inception score needs the classifier)")
        return None
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != INCEPTION_FC_SHAPE:
        raise MvdError(f"Inception-v3 (FID) weights: 'fc.weight' has shape {tuple(getattr(t, 'shape', ()))}, expected {INCEPTION_FC_SHAPE}")
    return t.detach().to(torch.float32).contiguous()


def fold_inception_fid(sd) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """name -> (folded weight rounded to bf16 [cout][cin][kh][kw], folded bias fp32) of every BasicConv2d: what both the kernels
    and the tests' restatement compute with"""
    sd = normalize_inception_fid_keys(sd)
    out = {}
    for e in INCEPTION_FID_CONVS:
        n = e[1]
        w, b = fold_batchnorm(sd[f"{n}.conv.weight"], sd[f"{n}.bn.weight"], sd[f"{n}.bn.bias"], sd[f"{n}.bn.running_mean"], sd[f"{n}.bn.running_var"])
        out[n] = (w.to(torch.bfloat16), b)
    return out


def pack_inception_fid(sd, device) -> Dict[str, torch.Tensor]:
    """``mvd_fid_set_weight`` slots: ``<name>.weight`` bf16 (``pack_slice_conv`` of the folded weight; the first layer's three input
    channels sit in the front end's ``FID_INPUT_CHANNELS``), ``<name>.bias`` fp32."""
    out = {}
    folded = fold_inception_fid(sd)
    for e in INCEPTION_FID_CONVS:
        name, src = e[1], e[2]
        w, b = folded[name]
        out[f"{name}.weight"] = pack_slice_conv(w, FID_INPUT_CHANNELS if src == "img" else 0).to(device).contiguous()
        out[f"{name}.bias"] = _f32(b, device)
    return out
