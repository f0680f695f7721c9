"""References for token merging, shared by tests/test_tome_cpu.py, tests/test_tome_host_cpu.py and the two
GPU test files.  Written from the algorithm (Bolya & Hoffman 2023; tomesd 0.1.x ``bipartite_soft_matching_random2d`` with
``use_rand=False``, ``sx = sy = 2``), not from the code under test:

(a) ``geometry`` / ``scores`` / ``decide`` / ``tables_from``: the decisions in fp64, with switches for the WRONG variants the
    tests must tell apart;
(b) ``merge_rows`` / ``unmerge_add``: the two data movements as the kernels are specified (fp32 sum in ascending token order, one
    rounding), on ANY slot table -- the GPU tests run them on the GPU's own table;
(c) ``tau`` / ``ambiguous``: the comparison margin of two fp32 scores and the tokens a test may leave out;
(d) ``tome_oracle``: a context manager under which the oracle's MAIN-pass forwards merge in front of ``attn1``.

Plain helper module, no fixtures; ``oracle/`` is not edited: (d) swaps two module attributes and puts them back."""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import sd21_unet as OU

# The setting of the engine parity tests: tests/test_tome_cpu.py shows that on the tiny topology every wrong variant (ToMe off,
# attn2 merged as well, the wrong level set, another row's table, merged src left at zero) is at least 4 * PARITY_BOUND_MAX away.
PARITY_SETTING = dict(ratio=0.5, max_downsample=1)
# The engine parity bound is 1.5 x the rel-L2 of the SAME inputs with ToMe off against the plain oracle, and never more than this:
PARITY_BOUND_MAX = 3e-2


# ------------------------------------------------------------------------------------------------------------ (a) decisions
def geometry(H, W, *, dst_bottom_right=False, drop_odd_row=False):
    """(dst tokens, src tokens) of an H x W map, long tensors: dst = the top-left token of every complete 2 x 2 cell in raster order
    of the cells, src = every other token, ascending.  WRONG on purpose: ``dst_bottom_right`` -- the cell's other corner;
    ``drop_odd_row`` -- an odd last row is neither (its tokens are missing from src)."""
    ys, xs = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
    o = 1 if dst_bottom_right else 0
    dst = ((2 * ys + o) * W + 2 * xs + o).reshape(-1)
    is_dst = torch.zeros(H * W, dtype=torch.bool)
    is_dst[dst] = True
    src = torch.nonzero(~is_dst).reshape(-1)
    if drop_odd_row and H % 2:
        src = src[src < (H - 1) * W]
    return dst, src


def scores(x, H, W, **geo):
    """cosine scores (B, #src, #dst) in fp64 of a (B, H*W, C) map"""
    dst, src = geometry(H, W, **geo)
    m = x.to(torch.float64)
    m = m / m.norm(dim=-1, keepdim=True)
    return m[:, src] @ m[:, dst].transpose(1, 2)


def decide(sc, r, *, tie_high=False):
    """(node_max, best, merged mask) of scores (B, #src, #dst): best = argmax over dst (the lowest index on a tie), the r src with the
    largest node_max merged (the lower index on a tie).  WRONG on purpose: ``tie_high`` -- both ties to the higher index."""
    if tie_high:
        nd = sc.shape[-1]
        node_max, best = sc.flip(-1).max(dim=-1)
        best = nd - 1 - best
        order = (sc.shape[1] - 1 - torch.sort(-node_max.flip(-1), dim=-1, stable=True).indices)
    else:
        node_max, best = sc.max(dim=-1)
        order = torch.sort(-node_max, dim=-1, stable=True).indices
    merged = torch.zeros_like(node_max, dtype=torch.bool)
    merged.scatter_(1, order[:, :r], True)
    return node_max, best, merged


def tables_from(best, merged, H, W, *, neighbour_dst=False, **geo):
    """slot (B, H*W) long: the merged row of every token -- dst d -> d, merged src -> best, the p-th kept src -> #dst + p.
    WRONG on purpose: ``neighbour_dst`` -- a merged src is booked to the dst after its best."""
    dst, src = geometry(H, W, **geo)
    B, nd = best.shape[0], dst.numel()
    slot = torch.full((B, H * W), -1, dtype=torch.long)
    slot[:, dst] = torch.arange(nd)
    kept_rank = torch.cumsum((~merged).long(), dim=1) - 1
    b = (best + 1) % nd if neighbour_dst else best
    slot[:, src] = torch.where(merged, b, nd + kept_rank)
    return slot


def reference_tables(x, H, W, r, **wrong):
    """slot table (B, H*W) of the definition, from the map alone"""
    geo = {k: v for k, v in wrong.items() if k in ("dst_bottom_right", "drop_odd_row")}
    _, best, merged = decide(scores(x, H, W, **geo), r, tie_high=wrong.get("tie_high", False))
    return tables_from(best, merged, H, W, neighbour_dst=wrong.get("neighbour_dst", False), **geo)


# ------------------------------------------------------------------------------------------------------- (b) data movements
def merge_rows(x, slot, rows, *, dtype=torch.float32, use_sum=False):
    """(B, rows, C): row j = the sum of the tokens with slot == j, accumulated in ``dtype`` ONE MEMBER AT A TIME in ascending token
    order, divided by the count, rounded once to x's dtype.  Tokens with slot < 0 belong to no row.  WRONG on purpose: ``use_sum``."""
    B, N, C = x.shape
    out = torch.zeros(B, rows, C, dtype=dtype)
    for b in range(B):
        s = slot[b].long()
        tok = torch.nonzero(s >= 0).reshape(-1)
        order = tok[torch.sort(s[tok], stable=True).indices]                  # by row, ascending token inside a row
        srt = s[order]
        count = torch.bincount(srt, minlength=rows)
        start = torch.cumsum(count, 0) - count
        rank = torch.arange(order.numel()) - start[srt]
        xb = x[b].to(dtype)
        acc = torch.zeros(rows, C, dtype=dtype)
        for k in range(int(count.max())):
            sel = rank == k
            if k == 0:
                acc[srt[sel]] = xb[order[sel]]
            else:
                acc[srt[sel]] = acc[srt[sel]] + xb[order[sel]]
        out[b] = acc if use_sum else acc / count.clamp_min(1).to(dtype)[:, None]
    return out.to(x.dtype)


def unmerge(t, slot, *, neighbour_row=False):
    """(B, H*W, C): every token takes row slot[token] of t.  WRONG on purpose: ``neighbour_row`` -- the slot of the next token."""
    s = slot.long()
    if neighbour_row:
        s = torch.roll(s, -1, dims=1)
    return torch.gather(t, 1, s.clamp_min(0)[:, :, None].expand(-1, -1, t.shape[-1]))


def unmerge_add(h, t, slot, **wrong):
    """bf16(float(h) + float(t[slot]))"""
    return (h.float() + unmerge(t, slot, **wrong).float()).to(h.dtype)


# ---------------------------------------------------------------------------------------------------------- (c) the margin
def tau(C):
    """Margin for comparing two scores computed as fp32 sums of C exact products, in any order, divided by fp32 norms.  With
    u = 2^-24: a recursive fp32 sum of C terms in any order errs by at most (C - 1) u sum|terms| (1 + O(C u)); for the dot product
    sum|x_i y_i| <= |x||y| (Cauchy-Schwarz), so its contribution to the score is at most (C - 1) u.  Each squared norm is a sum of C
    non-negative terms, relative error <= (C - 1) u, halved by the square root, plus one rounding of the root: (C + 1) u / 2 each,
    (C + 1) u for the two.  The product of the norms and the division round once each: 2 u.  One score: |error| <= (2 C + 2) u (the
    score itself is at most 1 in magnitude), which is below 2 (C + 4) u = tau / 2; a comparison of two scores is off by at most twice
    that, tau = 4 (C + 4) 2^-24."""
    return 4.0 * (C + 4) * 2.0 ** -24


def ambiguous(sc, r, t):
    """mask (B, #src) of the src whose decision a margin t cannot fix: the top two dst scores within t, or node_max within t of the
    selection boundary (the r-th / (r+1)-th largest node_max, whichever lies on the other side)."""
    top2 = torch.topk(sc, min(2, sc.shape[-1]), dim=-1).values
    amb = (top2[..., 0] - top2[..., -1] <= t) if sc.shape[-1] > 1 else torch.zeros(sc.shape[:2], dtype=torch.bool)
    node_max = top2[..., 0]
    srt = torch.sort(node_max, dim=-1, descending=True).values
    ns = node_max.shape[1]
    if 0 < r < ns:
        last_in, first_out = srt[:, r - 1:r], srt[:, r:r + 1]
        amb = amb | ((node_max >= last_in) & (node_max - first_out <= t)) | ((node_max <= first_out) & (last_in - node_max <= t))
    return amb


def seeded_map(B, H, W, C, seed, *, integer=False):
    """The inputs of the operator tests: a smooth field plus noise (neighbouring tokens correlate, as LayerNorm outputs of an image
    do), or small integers (every sum exact); bf16."""
    g = torch.Generator().manual_seed(seed)
    if integer:
        return torch.randint(-4, 5, (B, H * W, C), generator=g).to(torch.bfloat16)
    base = torch.randn(B, C, (H + 3) // 4 + 1, (W + 3) // 4 + 1, generator=g)
    smooth = F.interpolate(base, size=(H, W), mode="bilinear", align_corners=True)
    x = smooth + 0.7 * torch.randn(B, C, H, W, generator=g)
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C).to(torch.bfloat16).contiguous()


# ------------------------------------------------------------------------------------------------------ (d) the ToMe oracle
def block_merges(latent_hw, H, W, ratio, max_downsample):
    """r of a block whose map is H x W at a latent of latent_hw, 0 when it does not merge (tomesd's compute_merge)"""
    if H < 2 or W < 2:
        return 0
    down = math.ceil(math.sqrt((latent_hw[0] * latent_hw[1]) // (H * W)))
    if down > max_downsample:
        return 0
    return min(H * W - (H // 2) * (W // 2), int(H * W * ratio))


@contextlib.contextmanager
def tome_oracle(ratio, max_downsample=1, tables=None, *, merge_cross=False, levels_shift=0, roll_tables=False, zero_merged=False,
                neighbour_row=False, record=None, latent_hw=None):
    """Inside the block every MAIN-pass oracle forward (the forwards that do not pass ``capture``) merges in front of ``attn1`` of
    the eligible transformer blocks: n -> merge(n), attn1 (and the adapter's "self" hook) on the merged rows, un-merge, residual.
    ``tables``: ``{feature name: slot (B, H*W)}`` forces the decisions (the engine's own, from ``MVDEngine.tome_tables()``);
    otherwise they are the definition's on the oracle's own LayerNorm output.  ``record``: a dict that receives the tables used.
    ``latent_hw``: the latent size of a ``transformer_2d`` call made OUTSIDE ``unet_forward`` (one block on its own,
    tests/block_ref.py); inside a forward the forward's own sample decides, as ever, and the encoder pass never merges.
    WRONG on purpose: ``merge_cross`` -- attn2 runs on merged rows as well; ``levels_shift`` -- the eligibility test sees a latent
    2^shift times coarser per side: only the blocks of THAT level merge; ``roll_tables`` -- every image uses
    the table of the next image of the batch; ``zero_merged`` -- merged src get no attention output; ``neighbour_row`` -- every
    token un-merges from the row of the token after it (``unmerge(neighbour_row=True)``)."""
    orig_forward, orig_tf = OU.unet_forward, OU.transformer_2d
    state = {"latent": None if latent_hw is None else tuple(latent_hw)}      # (outside a forward; a forward sets its own)

    def forward(p, cfg, sample, timestep, text, attn_hook=None, block_hook=None, capture=None, **kw):
        prev = state["latent"]
        state["latent"] = tuple(sample.shape[-2:]) if capture is None else None
        try:
            return orig_forward(p, cfg, sample, timestep, text, attn_hook=attn_hook, block_hook=block_hook, capture=capture, **kw)
        finally:
            state["latent"] = prev

    def transformer(p, key, x, text, heads, groups, attn_hook, hook_name):
        lat = state["latent"]
        B, C, H, W = x.shape
        r = 0
        if lat is not None and levels_shift:
            r = block_merges((H, W), H, W, ratio, 1) if (lat[0] >> levels_shift, lat[1] >> levels_shift) == (H, W) else 0
        elif lat is not None:
            r = block_merges(lat, H, W, ratio, max_downsample)
        if r <= 0:
            return orig_tf(p, key, x, text, heads, groups, attn_hook, hook_name)
        N, nd = H * W, (H // 2) * (W // 2)
        res = x
        h = OU._gn(x, p, f"{key}.norm", groups, 1e-6)
        h = h.permute(0, 2, 3, 1).reshape(B, N, C)
        h = F.linear(h, p[f"{key}.proj_in.weight"], p[f"{key}.proj_in.bias"])
        b = f"{key}.transformer_blocks.0"
        n = F.layer_norm(h, (C,), p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], 1e-5)
        if tables is not None and hook_name in tables:
            slot = tables[hook_name].long().cpu().reshape(B, N)
        else:
            slot = reference_tables(n, H, W, r)
        if roll_tables:
            slot = torch.roll(slot, 1, dims=0)
        if record is not None:
            record[hook_name] = slot
        dst, _ = geometry(H, W)
        is_dst = torch.zeros(N, dtype=torch.bool)
        is_dst[dst] = True

        def attend(attn, kind, n_, ctx_self):
            m = merge_rows(n_, slot, N - r, dtype=n_.dtype)
            a = OU.attention(p, f"{b}.{attn}", m, m if ctx_self else text, heads)
            if attn_hook is not None:
                a = attn_hook(hook_name, kind, m, a)
            a = unmerge(a, slot, neighbour_row=neighbour_row)
            if zero_merged:
                a = torch.where(((slot < nd) & ~is_dst[None])[:, :, None], torch.zeros_like(a), a)
            return a
        h = h + attend("attn1", "self", n, True)
        n = F.layer_norm(h, (C,), p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], 1e-5)
        if merge_cross:
            h = h + attend("attn2", "cross", n, False)
        else:
            a = OU.attention(p, f"{b}.attn2", n, text, heads)
            if attn_hook is not None:
                a = attn_hook(hook_name, "cross", n, a)
            h = h + a
        n = F.layer_norm(h, (C,), p[f"{b}.norm3.weight"], p[f"{b}.norm3.bias"], 1e-5)
        f = F.linear(n, p[f"{b}.ff.net.0.proj.weight"], p[f"{b}.ff.net.0.proj.bias"])
        val, gate = f.chunk(2, dim=-1)
        f = F.linear(val * F.gelu(gate), p[f"{b}.ff.net.2.weight"], p[f"{b}.ff.net.2.bias"])
        h = h + f
        h = F.linear(h, p[f"{key}.proj_out.weight"], p[f"{key}.proj_out.bias"])
        return h.reshape(B, H, W, C).permute(0, 3, 1, 2) + res

    OU.unet_forward, OU.transformer_2d = forward, transformer
    try:
        yield
    finally:
        OU.unet_forward, OU.transformer_2d = orig_forward, orig_tf


# ------------------------------------------------------------------------------------ (e) the operator cases and their checks
# (B, H, W, C, r), seed.  The seeds of the small cases are those at which the reference has NO ambiguous src (tests/test_tome_cpu.py
# asserts it); the two large cases stay inside the 2 % cap.
SMALL_CASES = [((1, 8, 8, 320, 32), 2), ((3, 6, 10, 320, 20), 2), ((2, 7, 9, 640, 17), 2), ((2, 16, 16, 1280, 128), 7),
               ((1, 8, 8, 320, 1), 2), ((2, 6, 6, 320, 27), 2)]
LARGE_CASES = [((1, 64, 64, 320, 2048), 5), ((1, 96, 96, 320, 4608), 1)]
AMBIGUOUS_CAP = 0.02


def case_id(c):
    return "B{}_{}x{}_C{}_r{}".format(*c[0])


def check_decisions(x, H, W, r, score, best, slot, members=None, starts=None):
    """The GPU file's checks of one match + select result (CPU tensors) against the fp64 definition; returns (largest score error,
    ambiguous src).  AssertionError on the first failure."""
    B, N, C = x.shape
    t = tau(C)
    dst, src = geometry(H, W)
    nd, ns = dst.numel(), src.numel()
    sc = scores(x, H, W)
    node_max, ref_best, _ = decide(sc, r)
    amb = ambiguous(sc, r, t)
    assert int(amb.sum()) <= AMBIGUOUS_CAP * B * ns, f"{int(amb.sum())} ambiguous src of {B * ns}: the case checks too little"
    assert tuple(score.shape) == (B, ns) == tuple(best.shape), f"score / best of {tuple(score.shape)}, expected {(B, ns)}: every non-dst token is a src"
    # scores
    err = (score.double() - node_max).abs().max().item()
    assert err <= t / 2, f"score error {err:.3e} above tau / 2 = {t / 2:.3e}"
    # best
    best = best.long()
    assert ((best >= 0) & (best < nd)).all(), "best outside [0, #dst)"
    wrong = (best != ref_best) & ~amb
    assert not wrong.any(), f"{int(wrong.sum())} unambiguous src with the wrong best"
    # the table is a valid map
    slot = slot.long()
    assert tuple(slot.shape) == (B, N) and ((slot >= 0) & (slot < N - r)).all(), "slot outside [0, N')"
    assert (slot[:, dst] == torch.arange(nd)).all(), "dst j is not row j"
    s_slot = slot[:, src]
    merged = s_slot < nd
    assert (merged.sum(dim=1) == r).all(), f"merged src per image {merged.sum(dim=1).tolist()}, expected {r}"
    kept_rank = torch.cumsum((~merged).long(), dim=1) - 1
    assert (s_slot[~merged] == (nd + kept_rank)[~merged]).all(), "kept src do not take rows #dst, #dst + 1, .. in ascending token order"
    assert (s_slot[merged] == best[merged]).all(), "a merged src is not booked to its best dst"
    # the selection boundary
    srt = torch.sort(node_max, dim=-1, descending=True).values
    if 0 < r < ns:
        must_merge = node_max > srt[:, r:r + 1] + t
        must_keep = node_max < srt[:, r - 1:r] - t
        assert merged[must_merge].all(), "a src more than tau above the boundary was kept"
        assert not merged[must_keep].any(), "a src more than tau below the boundary was merged"
    # the member lists say what the table says
    if members is not None:
        members, starts = members.long(), starts.long()
        assert tuple(starts.shape) == (B, N - r + 1) and (starts[:, 0] == 0).all() and (starts[:, -1] == N).all(), "starts is no CSR of N tokens"
        assert (starts[:, 1:] > starts[:, :-1]).all(), "a merged row without a member"
        for b in range(B):
            row_of = torch.repeat_interleave(torch.arange(N - r), starts[b, 1:] - starts[b, :-1])
            assert (slot[b, members[b]] == row_of).all(), "a member is listed under a row that is not its slot"
            same = row_of[1:] == row_of[:-1]
            assert (members[b, 1:][same] > members[b, :-1][same]).all(), "members of a row do not ascend"
            assert torch.sort(members[b]).values.equal(torch.arange(N)), "members is no permutation of the tokens"
    return err, int(amb.sum())


def planted_ties(seed=11, B=1, H=8, W=8, C=320):
    """(x, r, (d_lo, d_hi), (s_lo, s_hi)): a map in which dst row d_hi is a copy of d_lo (every src that prefers them ties: the lower
    index must win) and src row s_hi a copy of s_lo (token-wise), with r such that exactly ONE of the two is merged: the lower."""
    x = seeded_map(B, H, W, C, seed)
    dst, src = geometry(H, W)
    d_lo, d_hi = 2, 9
    x[:, dst[d_hi]] = x[:, dst[d_lo]]
    t = tau(C)
    sc = scores(x, H, W)
    nm = sc.max(dim=-1).values[0]
    for s_lo in range(src.numel() - 1):                        # a src whose node_max is isolated from every other by more than tau
        s_hi = src.numel() - 1 - (s_lo % 5)
        if s_hi == s_lo:
            continue
        others = torch.ones_like(nm, dtype=torch.bool)
        others[s_lo] = others[s_hi] = False
        if (nm[others] - nm[s_lo]).abs().min() > 4 * t:
            break
    x[:, src[s_hi]] = x[:, src[s_lo]]
    nm = scores(x, H, W).max(dim=-1).values[0]
    others = torch.ones_like(nm, dtype=torch.bool)
    others[s_lo] = others[s_hi] = False
    assert (nm[others] - nm[s_lo]).abs().min() > 4 * t
    r = int((nm[others] > nm[s_lo]).sum()) + 1
    return x, r, (d_lo, d_hi), (int(s_lo), int(s_hi))


def check_planted_ties(x, H, W, r, ties, best, slot):
    (d_lo, d_hi), (s_lo, s_hi) = ties
    dst, src = geometry(H, W)
    nd = dst.numel()
    best, slot = best.long(), slot.long()
    ref_best = scores(x, H, W).max(dim=-1).indices
    prefers = (ref_best == d_lo) | (ref_best == d_hi)
    assert prefers.any(), "no src prefers the duplicated dst: the case checks nothing"
    assert (best[prefers] == d_lo).all(), "a tie between two dst did not go to the lower index"
    merged = slot[:, src] < nd
    assert merged[:, s_lo].all() and not merged[:, s_hi].any(), "a tie at the selection boundary did not go to the lower token"
    assert (merged.sum(dim=1) == r).all()


def check_moves(x, slot, rows, merged_out, h_in, t_in, h_out):
    """merge and un-merge + add, bit for bit against the restatement on the SAME table"""
    assert torch.equal(merged_out, merge_rows(x, slot, rows)), "merge differs from the fp32 mean in ascending token order"
    assert torch.equal(h_out, unmerge_add(h_in, t_in, slot)), "un-merge + add differs from bf16(float(h) + float(t[slot]))"


def emulate(x, H, W, r, *, t_in=None, h_in=None, perm=None, dst_bottom_right=False, drop_odd_row=False, tie_high=False, r_off=0,
            use_sum=False, neighbour_dst=False, neighbour_row=False):
    """The operators on the CPU as the kernels are specified -- fp32 scores from exact products (``perm``: the order in which the C
    products are added), decisions, tables, merge, un-merge + add -- with the op-level WRONG variants as switches.  Returns a dict
    with the arrays the GPU operators return."""
    B, N, C = x.shape
    geo = dict(dst_bottom_right=dst_bottom_right, drop_odd_row=drop_odd_row)
    dst, src = geometry(H, W, **geo)
    xf = x.float()
    if perm is not None:
        xf = xf[:, :, perm]
    a, d = xf[:, src], xf[:, dst]
    dot = torch.zeros(B, src.numel(), dst.numel())
    na, nb = torch.zeros(B, src.numel()), torch.zeros(B, dst.numel())
    for k in range(C):                                           # one fp32 addition per product, in order
        dot = dot + a[:, :, k:k + 1] * d[:, None, :, k]
        na = na + a[:, :, k] * a[:, :, k]
        nb = nb + d[:, :, k] * d[:, :, k]
    sc = dot / (na.sqrt()[:, :, None] * nb.sqrt()[:, None, :])
    node_max, best, merged = decide(sc, r + r_off, tie_high=tie_high)
    slot = tables_from(best, merged, H, W, neighbour_dst=neighbour_dst, **geo)
    rows = N - r - r_off
    out = dict(score=node_max, best=best, slot=slot, rows=rows)
    out["merged"] = merge_rows(x, slot, rows, use_sum=use_sum)
    if t_in is not None:
        t = F.pad(t_in, (0, 0, 0, max(rows - t_in.shape[1], 0)))[:, :rows]          # (r_off: the sequence is a row shorter / longer)
        out["h_out"] = unmerge_add(h_in, t, slot, neighbour_row=neighbour_row)
    return out
