"""Inputs whose correct result is one bit pattern, and the references that give it.

The tolerance tests (test_ops_gpu.py and its neighbours) bound max|err| by one bf16 ulp of the largest output.  A single wrong
operand element, one key dropped or two V rows swapped inside a tile, or a wrong rounding mode all stay below that bound.  The
problems here leave no such room:

* Integer problems (GEMM / convolution): activations are integers in [-3, 3], weights ternary, bias / row vector integers in
  [-8, 8], residual integers in [-16, 16], alpha in {1, 0.5, 2}.  Every product and partial sum is an integer or half-integer far
  below 2^24: exact in fp32 in any accumulation order, tiling or split-K.  The reference is fp64 on the CPU, rounded ONCE to
  bf16 (nearest even); the comparison is bitwise.  A share of the rows and columns is "tilted" -- correlated with a common sign
  vector along K, every element still inside the ranges above -- so that outputs reach the binades where integers (or
  half-integers) are bf16 ties (|x| >= 256, or >= 128 with alpha = 0.5): the rounding mode is visible.  Ties need
  3 K + 16 >= 256, so a problem with K < 128 has none; from K = 320 up the share is at least 1 % (test_exact_inputs_cpu.py).

* Routing problems (attention): keys are +-1 codes, query i is gain * code[pi(i)], V elements are +-(1 + m/128).  The softmax
  mass of every key but pi(i) is at most 2^-12 (checked here in fp64), which moves the output by less than 2^-11 relative --
  inside the half-ulp of bf16 -- so the correct output is v[pi(i)], bit for bit.  ``routing_pair`` gives two such problems for one
  two-problem launch, every K/V element of both with values of its own.

Plain helper module (like parity_util.py), no fixtures."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
STRENGTHS = (0.0, 0.25, 0.5, 0.75, 1.0)       # share of a tilted row's / column's elements that follow the common sign vector
ALPHAS = (1.0, 0.5, 2.0)


# ------------------------------------------------------------------------------------------------ comparison
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def describe_mismatch(got, want, what=""):
    """count of differing elements, the first differing index -- (row, column) or (b, y, x, channel) -- and got / want there"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{what}: got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    diff = _bits(got) != _bits(want)
    n = int(diff.sum())
    if n == 0:
        return f"{what}: equal"
    idx = tuple(int(i) for i in diff.nonzero()[0])
    return (f"{what}: {n} of {diff.numel()} elements differ; first at {idx}: got {got[idx].item()!r}, want {want[idx].item()!r}")


def same_bits(got, want):
    """(equal?, got on the CPU) -- bit patterns, so that -0 / +0 and NaN payloads count"""
    got = got.detach().cpu()
    return (got.shape == want.shape and got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))), got


# ------------------------------------------------------------------------------------------------ integer problems
def _gen(seed):
    return torch.Generator().manual_seed(0x5EED + 7919 * seed)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _tilted(g, rows, k, lo, hi, sign):
    """(rows, k) integers in [lo, hi]; in row r a share STRENGTHS[.] of the elements is sign[k] * |value|"""
    x = _ints(g, (rows, k), lo, hi)
    p = torch.tensor(STRENGTHS, dtype=torch.float64)[torch.randint(0, len(STRENGTHS), (rows,), generator=g)]
    coin = torch.rand(rows, k, generator=g, dtype=torch.float64) < p[:, None]
    return torch.where(coin, sign[None, :] * x.abs(), x)


def _sign(g, k):
    return torch.randint(0, 2, (k,), generator=g).double() * 2 - 1


@functools.lru_cache(maxsize=8)
def gemm_problem(m, n, k, groups=0, seed=0):
    """fp64 tensors: a (m, k), w (n, k), bias (n), rowvec (groups, n) or None, res (m, n)"""
    g = _gen(seed + m + 3 * n + 5 * k)
    s = _sign(g, k)
    return SimpleNamespace(a=_tilted(g, m, k, -3, 3, s), w=_tilted(g, n, k, -1, 1, s), bias=_ints(g, (n,), -8, 8),
                           rowvec=_ints(g, (groups, n), -8, 8) if groups else None, res=_ints(g, (m, n), -16, 16))


@functools.lru_cache(maxsize=8)
def conv_problem(B, H, W, cin, cout, sc0=0, sc1=0, seed=0):
    """fp64 tensors: x (B, H, W, cin), w (cout, cin, 3, 3), bias (cout), rowvec (B, cout), shortcut sources s0 / s1 (B, H, W, sc.)
    with the 1x1 weight wsc (cout, sc0 + sc1).  The common sign vector runs over the channels."""
    g = _gen(seed + B + 3 * H + 5 * W + 7 * cin + 11 * cout + 13 * sc0 + 17 * sc1)
    s = _sign(g, cin)
    x = _tilted(g, B * H * W, cin, -3, 3, s).reshape(B, H, W, cin)
    w = _tilted(g, cout * 9, cin, -1, 1, s).reshape(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()
    p = SimpleNamespace(x=x, w=w, bias=_ints(g, (cout,), -8, 8), rowvec=_ints(g, (B, cout), -8, 8), s0=None, s1=None, wsc=None)
    if sc0:
        ss = _sign(g, sc0 + sc1)
        src = _tilted(g, B * H * W, sc0 + sc1, -3, 3, ss).reshape(B, H, W, sc0 + sc1)
        p.s0, p.s1 = src[..., :sc0].contiguous(), (src[..., sc0:].contiguous() if sc1 else None)
        p.wsc = _tilted(g, cout, sc0 + sc1, -1, 1, ss)
    return p


def partial_sum_bound(k, alpha=2.0):
    """largest |value| any partial sum or epilogue term of an integer problem over K products can reach"""
    return abs(alpha) * (3 * k + 8 + 8) + 16


def bf(x64):
    """fp64 values that ARE bf16 values (inputs) -> bf16"""
    y = x64.float().to(torch.bfloat16)
    assert torch.equal(y.double(), x64), "not a bf16 value"
    return y


def f32(x64):
    y = x64.float()
    assert torch.equal(y.double(), x64), "not an fp32 value"
    return y


def round_once(y64, out_f32=False):
    """the one rounding of the contract: fp64 -> fp32 is exact here (asserted), fp32 -> bf16 rounds to nearest even"""
    y = f32(y64)
    return y if out_f32 else y.to(torch.bfloat16)


def epilogue(acc, bias=None, rowvec=None, rows_per_batch=0, res=None, alpha=1.0):
    """alpha * (acc + bias + rowvec[row // rows_per_batch]) + res in fp64; acc (..., n) with the rows flattened in order"""
    shape = acc.shape
    y = acc.reshape(-1, shape[-1])
    if bias is not None:
        y = y + bias
    if rowvec is not None:
        y = y + rowvec[torch.arange(y.shape[0]) // rows_per_batch]
    y = alpha * y
    if res is not None:
        y = y + res.reshape(y.shape)
    return y.reshape(shape)


def conv_acc(x, w, stride=1, upsample=False, asym=False):
    """fp64 3x3 convolution of NHWC x with w (cout, cin, 3, 3), padding 1 (asym: bottom / right only, stride 2) -> NHWC"""
    xi = x.permute(0, 3, 1, 2)
    if upsample:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    if asym:
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), w, stride=2, padding=0)
    else:
        y = F.conv2d(xi, w, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def tie_share(y64):
    """share of the values whose rounding to bf16 is an exact tie (low 16 bits of the fp32 pattern == 0x8000)"""
    return float(((f32(y64).contiguous().view(torch.int32) & 0xFFFF) == 0x8000).double().mean())


def truncate_to_bf16(y64):
    """the wrong rounding: chop the low 16 bits of the fp32 pattern"""
    b = f32(y64).contiguous().view(torch.int32) & -65536
    return b.view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ GEGLU
GEGLU_GATES = (10.0, 1.0, -0.5)      # constant gate values: gelu(10) == 10 in fp32 and in fp64 (exact products, ties included), two generic ones


def gelu64(c):
    return 0.5 * c * (1.0 + math.erf(c / math.sqrt(2.0)))


def gelu_f32_formula(c):
    """csrc/common.h gelu_erf_f evaluated in fp32 on the CPU (fma as one rounding of the fp64 result; 1 / x and exp2 correctly
    rounded where the hardware's are within one ulp)"""
    t32 = lambda v: torch.tensor(v, dtype=torch.float64).float()          # noqa: E731
    fma = lambda a, b, d: (a.double() * b.double() + d.double()).float()  # noqa: E731
    x = t32(c)
    ax = x.abs()
    t = 1.0 / fma(t32(0.3275911) * t32(0.70710678118654752), ax, t32(1.0))
    p = fma(t32(0.5) * t32(1.061405429), t, t32(0.5) * t32(-1.453152027))
    for coef in (1.421413741, -0.284496736, 0.254829592):
        p = fma(p, t, t32(0.5) * t32(coef))
    zl = ax * t32(0.84932180028801907)
    e = torch.exp2(-zl * zl)
    h = (ax * (p * t)) * e
    return float(torch.clamp(x, min=0.0) - h)


def round_f64_to_bf16(y64):
    """ONE rounding of arbitrary fp64 values to bf16 (nearest even on the 8-bit significand; normal range)"""
    mant, exp = torch.frexp(y64)
    return torch.ldexp(torch.round(mant * 256.0) / 256.0, exp).float().to(torch.bfloat16)


def ulp_distance(got, want):
    """bf16 tensors -> distance in units of the last place (sign-magnitude order)"""
    key = lambda t: (lambda b: torch.where(b >= 0, b, -(b & 0x7FFF)))(_bits(t).to(torch.int32))   # noqa: E731
    return (key(got) - key(want)).abs()


def geglu_problem(m, n_out, k, c, seed=0):
    """value half: integer GEMM (+ integer bias); gate half: zero weights, bias c.  Returns (a, w (2 n_out, k), bias (2 n_out),
    want bf16 (m, n_out)) with want = ONE rounding of val * gelu_fp64(c); w / bias in diffusers' order (value rows, then gate)."""
    p = gemm_problem(m, n_out, k, 0, seed)
    w = torch.cat([p.w, torch.zeros(n_out, k, dtype=torch.float64)], 0)
    bias = torch.cat([p.bias, torch.full((n_out,), c, dtype=torch.float64)], 0)
    val = p.a @ p.w.T + p.bias
    return p.a, w, bias, val, round_f64_to_bf16(val * gelu64(c))


def geglu_ok(got, want):
    """(no element differs by more than one bf16 ulp, share of differing elements <= 1 %, text)"""
    d = ulp_distance(got, want)
    share = float((d > 0).double().mean())
    return int(d.max()) <= 1, share <= 0.01, f"max ulp distance {int(d.max())}, {share:.4%} differ"


# ------------------------------------------------------------------------------------------------ routing problems (attention)
def _hash(*xs):
    h = torch.zeros((), dtype=torch.int64)
    for x, mul in zip(xs, (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F)):
        h = h + x * mul
    h = h & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    h = ((h ^ (h >> 12)) * 0x297A2D39) & 0xFFFFFFFF
    return h ^ (h >> 15)


def routing_values(B, heads, nk):
    """v (B, nk, heads * 64) fp64: +-(1 + m/128), m and the sign hashed from (batch, head, key, dim)"""
    b, j, h, d = torch.meshgrid(torch.arange(B), torch.arange(nk), torch.arange(heads), torch.arange(64), indexing="ij")
    x = _hash(b, h, j, d)
    v = (1.0 + (x & 127).double() / 128.0) * (1.0 - 2.0 * ((x >> 7) & 1).double())
    return v.reshape(B, nk, heads * 64)


def split_starts(nk, nsplit):
    """first key of every key range of the split-KV kernel (whole 64-key tiles, attention.hip kb0)"""
    tiles = (nk + 63) // 64
    return [64 * ((s * tiles) // nsplit) for s in range(nsplit)]


def must_hit(nk, nsplit=1):
    """keys pi has to reach: 0, nk - 1, both sides of every 64-key tile boundary and of every split boundary"""
    ks = {0, nk - 1}
    for t in list(range(64, nk, 64)) + split_starts(nk, nsplit)[1:]:
        ks.update((t - 1, t))
    return sorted(k for k in ks if 0 <= k < nk)


def routing_map(B, heads, nq, nk, nsplit=1, causal=False, seed=0):
    """pi (B, heads, nq) int64.  Per (batch, head): the must-hit keys first (rotated, so that few queries still reach all of
    them over the heads), then every other key in a seeded order of its own, then seeded repeats; the queries that take them
    are a seeded permutation too.  causal: pi(i) <= i, cycling through pi(i) = i, 0 and a seeded key below i."""
    g = _gen(1000 + seed + B + 3 * heads + 5 * nq + 7 * nk + 11 * nsplit)
    pi = torch.empty(B, heads, nq, dtype=torch.int64)
    must = must_hit(nk, nsplit)
    must_set = set(must)
    for b in range(B):
        for h in range(heads):
            if causal:
                i = torch.arange(nq)
                rnd = (torch.rand(nq, generator=g) * (i + 1)).long().clamp(max=nq - 1)
                kind = (i + b + h) % 3
                pi[b, h] = torch.where(kind == 0, i, torch.where(kind == 1, torch.zeros_like(i), torch.minimum(rnd, i)))
                continue
            r = ((b * heads + h) * nq) % len(must)
            first = must[r:] + must[:r]
            rest = [k for k in torch.randperm(nk, generator=g).tolist() if k not in must_set]
            order = (first + rest)[:nq]
            order += torch.randint(0, nk, (nq - len(order),), generator=g).tolist()
            pi[b, h, torch.randperm(nq, generator=g)] = torch.tensor(order)
    return pi


@functools.lru_cache(maxsize=4)
def routing_problem(B, heads, nq, nk, gain, prescaled=False, nsplit=1, causal=False, seed=0):
    """q (B, nq, C), k, v (B, nk, C) and want (B, nq, C) as bf16, C = heads * 64; stats: ``mass`` = log2 of the largest softmax
    mass off the chosen key, ``lift`` = per query, exp2-domain score of the chosen key minus the best score in the first 64
    keys of its key range (what the engine form's first-tile maximum is short of it).  Generic form: q = +-gain with
    scale = 0.125; prescaled: q = +-bf16(gain * QSCALE), scale = 0.  Asserts mass <= -12."""
    from mvd_amd.packing import QSCALE
    g = _gen(2000 + seed + heads + 3 * nk)
    codes = torch.randint(0, 2, (heads, nk, 64), generator=g).double() * 2 - 1          # each head its own set
    pi = routing_map(B, heads, nq, nk, nsplit, causal, seed)
    amp = float(torch.tensor(gain * QSCALE).to(torch.bfloat16)) if prescaled else float(gain)
    unit = 1.0 if prescaled else 0.125 * LOG2E                                          # exp2-domain score per unit of q . k
    hh = torch.arange(heads)[None, :, None]
    qh = amp * codes[hh, pi]                                                            # (B, heads, nq, 64)
    s = torch.einsum("bhqd,hkd->bhqk", qh, codes) * unit
    if causal:
        s = s.masked_fill(torch.arange(nk)[None, :] > torch.arange(nq)[:, None], -math.inf)
    chosen = s.gather(3, pi[..., None])
    off = torch.exp2(s - chosen).sum(-1) - 1.0                                          # (the chosen key itself contributes 1)
    starts = torch.tensor(split_starts(nk, nsplit))
    r0 = starts[torch.bucketize(pi, starts, right=True) - 1]                            # first key of the chosen key's range
    win = r0[..., None] + torch.arange(64)                                              # (B, heads, nq, 64)
    first = s.gather(3, win.clamp(max=nk - 1)).amax(-1)
    lift = chosen[..., 0] - first
    mass = math.log2(max(float(off.max()), 2.0 ** -200))
    assert mass <= -12.0, f"off-target softmax mass 2^{mass:.1f}"
    v = routing_values(B, heads, nk)
    want = v.reshape(B, nk, heads, 64).permute(0, 2, 1, 3)[torch.arange(B)[:, None, None], hh, pi]   # (B, heads, nq, 64)
    q = qh.permute(0, 2, 1, 3).reshape(B, nq, heads * 64)
    k = codes.permute(1, 0, 2).reshape(1, nk, heads * 64).expand(B, nk, heads * 64)
    return SimpleNamespace(q=bf(q), k=bf(k.contiguous()), v=bf(v), want=bf(want.permute(0, 2, 1, 3).reshape(B, nq, heads * 64)),
                           pi=pi, mass=mass, lift=lift, scale=0.0 if prescaled else 0.125)


@functools.lru_cache(maxsize=8)
def routing_pair(E0, E1, heads, nq0, nk0, nq1, nk1, gain, prescaled=False, nsplit=1):
    """Two routing problems for ONE launch of two problems (MvdAttnArgs::nprob = 2): problem i has E_i K/V elements with nq_i
    queries and nk_i keys each.  ``routing_values`` hashes V from (element, head, key, dim) alone, so two ``routing_problem``s of
    one shape hold the same V and a launch that read problem 0's V for problem 1 would return the wanted bits; here ONE
    ``routing_values`` call over the E0 + E1 elements of both problems gives every element values of its own, and ``want`` is
    taken from them.  The key codes and the routing maps differ too (seeds 0 and 1; asserted).  The per-problem checks are
    ``routing_problem``'s: off-target mass <= 2^-12, ``lift``, ``must_hit(nk_i, nsplit)``.  Returns (p0, p1), fields as
    ``routing_problem``'s."""
    ps = [routing_problem(E, heads, nq, nk, gain, prescaled, nsplit, False, seed) for seed, (E, nq, nk) in enumerate(((E0, nq0, nk0), (E1, nq1, nk1)))]
    v = routing_values(E0 + E1, heads, max(nk0, nk1))
    out = []
    for p, vv in zip(ps, (v[:E0, :nk0], v[E0:, :nk1])):
        E, nk, _ = vv.shape
        want = vv.reshape(E, nk, heads, 64).permute(0, 2, 1, 3)[torch.arange(E)[:, None, None], torch.arange(heads)[None, :, None], p.pi]
        out.append(SimpleNamespace(q=p.q, k=p.k, v=bf(vv.contiguous()), want=bf(want.permute(0, 2, 1, 3).reshape(E, -1, heads * 64)), pi=p.pi,
                                   mass=p.mass, lift=p.lift, scale=p.scale))
    n, e, m = min(nk0, nk1), min(E0, E1), min(nq0, nq1)
    assert not torch.equal(out[0].k[:e, :n], out[1].k[:e, :n]), "the two problems share their key codes"
    assert not torch.equal(out[0].pi[:e, :, :m], out[1].pi[:e, :, :m]), "the two problems share their routing map"
    assert not torch.equal(out[0].v[:e, :n], out[1].v[:e, :n])
    return tuple(out)


# gains of the three regimes: LAZY -- the engine form may keep its first tile's maximum (lift <= 90; the kernel re-runs from a
# denominator of 2^64 on, so some of these workgroups do re-run); STRICT_LAZY -- lift < 60, below that bound for every
# query: the unchecked loop's result is what gets stored; RERUN -- lift >= 140 for some query: the unchecked loop overflows
LAZY, STRICT_LAZY, RERUN = 8.0, 6.0, 16.0


def attention_reference(q, k, v, heads, unit, causal=False, swap=None, drop=None):
    """fp64 softmax attention in the exp2 domain (scores q . k * unit) on (B, n, heads * 64) tensors -- the CPU emulation the
    mutation tests bend: ``swap=(j1, j2)`` exchanges two V rows, ``drop=j`` leaves key j out"""
    B, nq, C = q.shape
    nk = k.shape[1]
    sp = lambda t, n: t.double().reshape(B, n, heads, 64).transpose(1, 2)   # noqa: E731
    s = sp(q, nq) @ sp(k, nk).transpose(2, 3) * unit
    if causal:
        s = s.masked_fill(torch.arange(nk)[None, :] > torch.arange(nq)[:, None], -math.inf)
    if drop is not None:
        s[..., drop] = -math.inf
    vv = sp(v, nk).clone()
    if swap is not None:
        vv[:, :, list(swap)] = vv[:, :, list(swap[::-1])]
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return ((p / p.sum(-1, keepdim=True)) @ vv).transpose(1, 2).reshape(B, nq, C)


# ------------------------------------------------------------------------------------------------ shared by the GPU files
@functools.lru_cache(maxsize=8)
def gemm_acc(m, n, k, groups=0, seed=0):
    """a . w^T of gemm_problem in fp64, computed once for all the kernel forms that are compared with it"""
    p = gemm_problem(m, n, k, groups, seed)
    return p.a @ p.w.T


def assert_same_bits(got, want, what=""):
    """the one comparison of the exact tests: torch.equal on the bit patterns, with a message that locates the fault"""
    ok, got = same_bits(got, want)
    assert ok, describe_mismatch(got, want, what)


# ------------------------------------------------------------------------------------------------ views of wider buffers
SENTINEL_BITS = {torch.bfloat16: 0x5A5A, torch.float32: 0x5A5A5A5A}     # 1.5e16: finite, beyond any partial_sum_bound


def sentinel(dtype):
    """the guard value of ``dtype`` (bf16 / fp32) as a 0-d tensor: one known bit pattern that no reference value has"""
    return torch.tensor(SENTINEL_BITS[dtype], dtype=torch.int16 if dtype == torch.bfloat16 else torch.int32).view(dtype)


def embed(t, ld, off, fill):
    """(rows, n) tensor -> a new (rows, ld) buffer of the same dtype and device with ``t`` in columns [off, off + n) and ``fill`` (a
    number, NaN included, or a 0-d tensor such as ``sentinel``) everywhere else; the operand is then ``buf[:, off:off + n]``"""
    rows, n = t.shape
    assert 0 <= off and off + n <= ld, (off, n, ld)
    buf = torch.empty(rows, ld, dtype=t.dtype, device=t.device)
    buf[:] = fill.to(t.device) if torch.is_tensor(fill) else fill
    buf[:, off:off + n] = t
    return buf


def outside_unchanged(buf, before, off, n):
    """the guard columns of ``buf`` -- everything outside [off, off + n) -- hold the bit patterns they hold in ``before``"""
    b, a = _bits(buf.detach().cpu()), _bits(before.detach().cpu())
    return b.shape == a.shape and torch.equal(b[:, :off], a[:, :off]) and torch.equal(b[:, off + n:], a[:, off + n:])


def dev(x64):
    """fp64 bf16-valued tensor (or None) -> bf16 on the GPU"""
    return None if x64 is None else bf(x64).contiguous().cuda()


def dev32(x64):
    return None if x64 is None else f32(x64).contiguous().cuda()
