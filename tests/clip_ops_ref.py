"""fp64 references, inputs and bounds of the CLIP towers' and the VAE's own kernels (mvd_amd/ops.py: clip_add_ln, clip_act,
text_embed, vit_patchify, vit_embed_ln, vit_fold, clip_l2norm, clip_score.pool_project, vae_pointwise), shared by
tests/test_clip_ops_cpu.py (which shows on the CPU that these data tell right from wrong) and tests/test_clip_ops_gpu.py.

Bounds -- none is new:

* fp32 LayerNorm outputs: ``conditioning_ref.layernorm_bound`` (4 x the two-pass fp32 emulation's worst error against fp64, per case);
  the bf16 output is the round-to-nearest-even of the fp32 output, bit for bit.
* element-wise fp32 (embed, fold, the x += delta write-back): bit equality with torch's fp32 add on the CPU -- one IEEE add each.
* activation: per element (2^-8 + 2^-14) |want| + 1e-30 (tests/test_vae_ops_gpu.py::test_softmax_rows); the mean of
  (got - want) / ulp_bf16(want) over |want| >= 2^-20 within 6 / sqrt(12 N): unbiased rounding has deviation 1 / sqrt(12) ulp.
* pool / project / l2norm: 1e-5 against fp64 (tests/test_clip_score_gpu.py).
* pointwise, patchify: integer data whose fp32 sums are exact (asserted here) -> bit equality.
* statistics: the spike probes of stat_probe.py on the ``Rows`` layout.  The row a kernel normalises is a SUM of two inputs (x + delta,
  [class | patches] + position, hidden + delta): the background is N(0, 1) in the first and N(0, 1) / 8 in the second, and the spike
  sits in the first or the second by (row + launch + flip) parity, so the statistic has to be taken after the add.

Plain helper module (like conditioning_ref.py / stat_probe.py): no fixtures, no tests."""
import math

import torch

from tests import clip_vision_ref as V
from tests import conditioning_ref as CR
from tests import stat_probe as P

EPS = 1e-5
LN_MAXH = 2048                                   # LN_MAXCH * 256 of clip_layer.h, PP_MAXH of vision.hip
ADD_LN_H = (64, 128, 768, 1024, 1280, 2048)      # 16 float4 chunks for 64 lanes, the towers' widths, 5 chunks per lane, all 8
ADD_LN_ROWS = (1, 4, 5, 65)                      # one wave per row, four rows per workgroup, a ragged last group
EMBED_LN_CASES = [(B, T, H) for B, T in ((1, 5), (3, 17), (2, 50)) for H in (128, 768, 2048)]
EMBED_LN_PROBE_H = (128, 768, 2048)
POOL_PROBE_H = (64, 1280, 2048)
PROBE_ROWS = 65                                  # ceil(2048 / 65) = 32 = stat_probe.BUDGET launches
SENTINEL = 12288.0                               # (a bf16 value)


def gen(*key):
    return torch.Generator().manual_seed(0xC11 + sum(int(k) * m for k, m in zip(key, (1, 131, 7919, 104729))))


def rne_bf16(t):
    """fp32 -> bf16 round-to-nearest-even (torch's conversion)"""
    return t.float().to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


# ------------------------------------------------------------------------------------------------ LayerNorm-type kernels
def affine(H, seed=0):
    g = gen(H, seed, 1)
    return (1 + 0.2 * torch.randn(H, generator=g)).float(), (0.1 * torch.randn(H, generator=g)).float()


def add_ln_case(H, rows, seed=0):
    """x, delta (rows, H) fp32 with a row mean and a delta of the residual stream's proportions, gamma, beta"""
    g = gen(H, rows, seed)
    x = (1.5 * torch.randn(rows, H, generator=g) + 0.3).float()
    delta = (0.4 * torch.randn(rows, H, generator=g)).float()
    return (x, delta) + affine(H, seed)


def add_ln_ref(x, delta, gamma, beta, eps=EPS):
    """-> (x afterwards = fl32(x + delta) or x itself, y in fp64, the fp32 bound of this case)"""
    s = x if delta is None else x + delta
    return s, CR.layernorm_f32(s, gamma, beta, eps), CR.layernorm_bound(s, gamma, beta, eps)


def embed_ln_case(B, T, H, seed=0):
    """patch_out (B * (T - 1), H), cls (H,), pos (T, H): distinct random rows, class and position tables of their own"""
    g = gen(B, T, H, seed)
    return ((torch.randn(B * (T - 1), H, generator=g)).float(), (0.3 * torch.randn(H, generator=g) + 0.2).float(),
            (0.3 * torch.randn(T, H, generator=g)).float()) + affine(H, seed + 1)


def embed_rows(patch_out, cls, pos, B, mutate=None):
    """fl32([class | patches] + position), (B * T, H).  ``mutate``: 'cls_from_patch0' -- the class row taken from patch 0;
    'prev_image' -- image b reading image b - 1's patches (what the kernel must NOT do)."""
    T, H = pos.shape
    po = patch_out.reshape(B, T - 1, H)
    if mutate == "prev_image":
        po = po.roll(1, 0)
    first = po[:, :1] if mutate == "cls_from_patch0" else cls.expand(B, 1, H)
    return (torch.cat([first, po], 1) + pos).reshape(B * T, H)


def probe_slots(H, rows=PROBE_ROWS):
    """(launches, rows): the hot column of every row in every launch -- every column of the width comes up (H <= EXHAUSTIVE_MAX)"""
    return P.schedule(H, rows, P.exhaustive(H), 1, seed=H)


def probe_pair(H, rows, hot, launch, flip=0, seed=0):
    """(first, second) fp32 (rows, H) whose fp32 sum is the probed row: backgrounds N(0, 1) and N(0, 1) / 8 (bf16 values), the spike
    in ``first`` where (row + launch + flip) is even, in ``second`` elsewhere"""
    first = P.background(rows, H, seed).float().clone()
    second = (P.background(rows, H, seed + 1).float() / 8).clone()
    r = torch.arange(rows)
    in_second = (r + launch + flip) % 2 == 1
    v = P.spike(H)
    first[r[~in_second], hot[~in_second]] = v
    second[r[in_second], hot[in_second]] = v
    return first, second


def probe_affine(H):
    g = gen(H, 5)
    return (1 + 0.1 * torch.randn(H, generator=g)).float(), (0.1 * torch.randn(H, generator=g)).float()


# ------------------------------------------------------------------------------------------------ index kernels
def text_embed_case(rows, T, H, vocab=50, positions=77, seed=0):
    """ids (rows,) int32 in [0, vocab) with 0 and vocab - 1 among them, tok (vocab, H), pos (positions, H)"""
    g = gen(rows, T, H, seed)
    ids = torch.randint(0, vocab, (rows,), generator=g).to(torch.int32)
    ids[0], ids[-1] = 0, vocab - 1
    return ids, (0.02 * torch.randn(vocab, H, generator=g)).float(), (0.01 * torch.randn(positions, H, generator=g)).float()


def text_embed(ids, tok, pos, T, mutate=None):
    """tok[clamp(ids)] + pos[row % T] as one fp32 add; ``mutate`` 'pos_row': position row ``row`` instead (clamped to the table)"""
    rows = ids.shape[0]
    r = torch.arange(rows)
    pr = r.clamp(max=pos.shape[0] - 1) if mutate == "pos_row" else r % T
    return tok[ids.long().clamp(0, tok.shape[0] - 1)] + pos[pr]


def patch_rows_bf16(pv, P_, mutate=None):
    """clip_vision_ref.patch_rows rounded to bf16, zero padded to the next multiple of 64 columns; ``mutate`` 'pyx_c': (py, px, c) order"""
    B, C, S, _ = pv.shape
    g = S // P_
    if mutate == "pyx_c":
        rows = pv.reshape(B, C, g, P_, g, P_).permute(0, 2, 4, 3, 5, 1).reshape(B * g * g, C * P_ * P_)
    else:
        rows = V.patch_rows(pv, P_)
    kp = (3 * P_ * P_ + 63) // 64 * 64
    out = torch.zeros(rows.shape[0], kp, dtype=torch.bfloat16)
    out[:, :rows.shape[1]] = rne_bf16(rows)
    return out


# ------------------------------------------------------------------------------------------------ activation
ACT_N = 65 * 1024          # >= 65536, and room for the largest partial launch (8 * 8193 elements) with a sentinel behind it


def act_inputs(n=ACT_N, seed=0):
    """n fp32 values uniform over [-8, 8], the two ends included"""
    x = (torch.rand(n, generator=gen(n, seed), dtype=torch.float64) * 16 - 8).float()
    x[0], x[1] = -8.0, 8.0
    return x


def act64(x, act):
    """fp64: act 0 gelu (erf form, the tail through erfc: no cancellation), 1 quick_gelu"""
    x = x.double()
    if act == 0:
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    return x * torch.sigmoid(1.702 * x)


def act_f32(x, act, c=1.702, tanh=False):
    """the kernel's formula in torch fp32; ``c`` / ``tanh``: the wrong constant and the wrong GELU the bias test must catch"""
    x = x.float()
    if act == 1:
        return x / (1.0 + torch.exp(-torch.tensor(c, dtype=torch.float32) * x))
    if tanh:
        return torch.nn.functional.gelu(x, approximate="tanh")
    return 0.5 * x * torch.special.erfc(-x * 0.70710678118654752)


def act_bound(want):
    return (2.0 ** -8 + 2.0 ** -14) * want.abs() + 1e-30


def ulp_bf16(want):
    """bf16 ulp of the binade of |want| (fp64)"""
    _, e = torch.frexp(want.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(want), e - 8)


def act_bias(got, want):
    """(mean of (got - want) / ulp_bf16(want) over |want| >= 2^-20, the bound 6 / sqrt(12 N), N)"""
    got, want = got.double().cpu(), want.double().cpu()
    sel = want.abs() >= 2.0 ** -20
    n = int(sel.sum())
    return ((got - want) / ulp_bf16(want))[sel].mean().item(), 6.0 / math.sqrt(12.0 * n), n


# ------------------------------------------------------------------------------------------------ pool / project / l2norm
def pool_project(hidden, delta, gamma, beta, w, eps=EPS):
    """token 0 of hidden (+ delta), LayerNorm, bias-free projection -> (raw, normalised), fp64"""
    row = (hidden if delta is None else hidden + delta)[:, 0]
    y = CR.layernorm_f32(row, gamma, beta, eps) @ w.double().T
    return y, y / y.norm(dim=-1, keepdim=True)


def l2norm(x, drop=None):
    """x / ||x||_2 per row, fp64; ``drop`` (rows,): the column left out of the sum of squares (a fault for the CPU file)"""
    x = x.double()
    sq = (x * x).sum(-1, keepdim=True)
    if drop is not None:
        sq = sq - x.gather(1, drop[:, None]) ** 2
    return x / sq.sqrt()


def l2norm_case(rows, dim, seed=0):
    """(x (rows, dim) fp32 with one spike per row, its columns)"""
    hot = torch.arange(rows) % dim
    return P.with_spike(P.background(rows, dim, seed + dim), hot).float(), hot


# ------------------------------------------------------------------------------------------------ VAE pointwise
def pointwise_case(B, cin, cout, hw, seed=0):
    """integer-valued x (B, cin, hw), w (cout, cin), bias (cout,): every partial sum is an integer below 2^24, so fp32 is exact in any
    order and with or without fma"""
    g = gen(B, cin, cout, hw + seed)
    x = torch.randint(-64, 65, (B, cin, hw), generator=g).float()
    w = torch.randint(-16, 17, (cout, cin), generator=g).float()
    bias = torch.randint(-100, 101, (cout,), generator=g).float()
    assert bias.abs().max().item() + cin * 16 * 64 < 2 ** 24
    return x, w, bias


def pointwise(x, w, bias):
    y = torch.einsum("oc,bcp->bop", w.double(), x.double()) + bias.double()[None, :, None]
    assert y.abs().max().item() < 2 ** 24 and torch.equal(y, y.round())
    return y.float()
