"""Spike problems for the kernels that compute a statistic, and the check that reads them.

The tolerance tests bound max|err| by 2^-7 * max|ref| on Gaussian inputs.  A statistic over N such elements moves by about 1/N when
one element is dropped, counted twice or handed to the neighbouring group: far below that bound (test_stat_probe_cpu.py states it
as a test).  A spike problem leaves no such room.  Every statistic DOMAIN -- one (image, group) of GroupNorm, one row of LayerNorm,
one pixel of the reference normalisation -- is a background of bf16 N(0, 1) values in which ONE hot element is set to V, the
smallest power of two with V^2 >= 8 N: the spike then carries at least 8/9 of the domain's sum of squares, so a statistic that
misses it, sees it twice or books it elsewhere changes every output of the domain by tens of per cent.

Everything here works on the DOMAIN-MAJOR view of a tensor: (domains, N), position p of a domain along the second axis.  A layout
object (``GN``, ``RefNorm``, ``Rows``) converts between that view and the operator's own layout.  The reference is the plain
normalisation of the same bf16 inputs in fp64.  The check has two tiers per domain, both at the project's 2^-7:

* the hot output:        |got - want| <= 2^-7 * |want|
* every other output:    |got - want| <= 2^-7 * max|want| over the domain's non-hot elements + 1e-6   (the floor of ``close``)

One launch probes one position per domain, so the hot position cycles over domains and launches (``schedule``): a list of
positions that MUST be hot somewhere -- all of them for a domain of at most 8192 elements, else the list ``must_hit`` builds from
the launch plan -- is dealt to the (launch, domain) slots so that every channel of every group comes up, and positions from a
fixed seed fill the rest.  The schedule is
a pure function of its arguments, so the CPU file enumerates what the GPU file probes.  A wrong divisor (N - 1 for N) is NOT seen
by this design; the small-N tolerance tests see that.

Plain helper module (like exact_util.py), no fixtures and no tests."""
import functools
import math

import torch

TOL = 2.0 ** -7
FLOOR = 1e-6
BUDGET = 32                 # launches per case at most
EXHAUSTIVE_MAX = 8192       # domains up to this size have every position hot somewhere
FAULTS = ("drop", "twice", "novar", "neighbour")
GELU_ERR = 1.5e-7           # |error| of csrc/common.h gelu_erf_f, as documented there


def spike(n):
    """the smallest power of two V with V^2 >= 8 n"""
    v = 1.0
    while v * v < 8 * n:
        v *= 2.0
    return v


# ------------------------------------------------------------------------------------------------ layouts
class Rows:
    """(rows, c): a row is a domain (LayerNorm and its folds)"""

    def __init__(self, rows, c):
        self.ndom, self.n, self.groups = rows, c, 1

    def to_dom(self, t):
        return t

    def from_dom(self, x):
        return x

    def affine(self, gamma, beta):
        return gamma.double()[None], beta.double()[None]

    def where(self, d, p):
        return f"row {d}, column {p}"


class GN:
    """(B, hw, C) with C = groups * cg: domain b * groups + g holds (pixel, channel-in-group) at position pixel * cg + cc"""

    def __init__(self, B, hw, C, groups=32):
        self.B, self.hw, self.C, self.groups, self.cg = B, hw, C, groups, C // groups
        self.ndom, self.n = B * groups, hw * (C // groups)

    def to_dom(self, t):
        return t.reshape(self.B, self.hw, self.groups, self.cg).permute(0, 2, 1, 3).reshape(self.ndom, self.n)

    def from_dom(self, x):
        return x.reshape(self.B, self.groups, self.hw, self.cg).permute(0, 2, 1, 3).reshape(self.B, self.hw, self.C).contiguous()

    def affine(self, gamma, beta):
        """per-channel (C,) vectors -> (groups, n) fp64, the factor and the offset of every position of a group's domain"""
        f = lambda v: v.double().reshape(self.groups, 1, self.cg).expand(self.groups, self.hw, self.cg).reshape(self.groups, self.n)  # noqa: E731
        return f(gamma), f(beta)

    def where(self, d, p):
        b, g = divmod(d, self.groups)
        return f"image {b}, group {g}, pixel {p // self.cg}, channel {g * self.cg + p % self.cg} (position {p})"


class RefNorm:
    """(B, hw, c): pixel p is a domain; it holds (image, channel) at position b * c + ch"""

    def __init__(self, B, hw, c):
        self.B, self.hw, self.c, self.groups = B, hw, c, 1
        self.ndom, self.n = hw, B * c

    def to_dom(self, t):
        return t.permute(1, 0, 2).reshape(self.ndom, self.n)

    def from_dom(self, x):
        return x.reshape(self.hw, self.B, self.c).permute(1, 0, 2).contiguous()

    def where(self, d, p):
        return f"pixel {d}, image {p // self.c}, channel {p % self.c}"


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=2)
def background(ndom, n, seed=0, shift=0.0):
    """(ndom, n) bf16 on the CPU: N(0, 1) (+ shift) from a fixed seed -- one per case, shared by its launches"""
    g = torch.Generator().manual_seed(0x57A7 + 7919 * seed + ndom + 3 * n)
    return (torch.randn(ndom, n, generator=g) + shift).to(torch.bfloat16)


def with_spike(bg, hot, v=None):
    """a copy of the domain-major background with position hot[d] of domain d set to V"""
    x = bg.clone()
    x[torch.arange(x.shape[0], device=x.device), hot.to(x.device)] = spike(x.shape[1]) if v is None else v
    return x


def exhaustive(n):
    return tuple((-1, p) for p in range(n))


def must_hit(plan, hw, cg, c0=0, capacity=None):
    """Positions a GroupNorm case has to probe when its domain is too large for all of them: ``(entries, info)``.  An entry is
    (group or -1, position); group -1 = any domain.  Pixels, in order of priority: 0, 1, hw - 2, hw - 1; both sides of every
    boundary of the statistics partition (slice kernel: ``npl`` pixels per pass; two-kernel form: ``rows_per_chunk``); the first
    ``R`` rows of every chunk (each thread's first sample is its shift); both sides of every boundary of the apply kernel's
    ``apply_rows``.  Every pixel is crossed with every channel index of the group.  With ``c0`` (two sources), the channels on
    both sides of c0 at the edge pixels and the first boundary, in the groups that own them.  ``capacity`` (slots): when the
    cross product does not fit, every pixel is listed once as (-2, pixel) -- ``schedule`` picks its channel so that every
    channel of every group still comes up --, the channels either side of c0 keep pixels 0 and hw - 1 only, and pixels of the
    lowest priority are dropped from the end if even that does not fit; ``info`` says what happened: pixels, kept, channels
    (per pixel), full."""
    sides = lambda step: [q for t in range(step, hw, step) for q in (t - 1, t)]      # noqa: E731
    px = [0, 1, hw - 2, hw - 1]
    if plan["form"] == "slice":
        stat_step = plan["npl"]
        px += sides(stat_step)
    else:
        stat_step = plan["rows_per_chunk"]
        px += sides(stat_step)
        px += [t + r for t in range(0, hw, stat_step) for r in range(plan["R"])]
        px += sides(plan["apply_rows"])
    px = list(dict.fromkeys(q for q in px if 0 <= q < hw))
    room = capacity
    edges = list(dict.fromkeys(q for q in [0, 1, hw - 2, hw - 1, stat_step - 1, stat_step] if 0 <= q < hw))
    full = room is None or len(px) * cg + (2 * len(edges) if c0 else 0) <= room
    special = []
    if c0:
        gs, off = divmod(c0, cg)
        owners = [(gs, off - 1), (gs, off)] if off else [(gs - 1, cg - 1), (gs, 0)]
        for q in edges if full else [0, hw - 1]:
            special += [(g, q * cg + cc) for g, cc in owners]
    if full:
        entries = [(-1, q * cg + cc) for q in px for cc in range(cg)]
        return tuple(special + entries), dict(pixels=len(px), kept=len(px), channels=cg, full=True)
    kept = min(len(px), room - len(special))
    return tuple(special + [(-2, q) for q in px[:kept]]), dict(pixels=len(px), kept=kept, channels=1, full=False)


@functools.lru_cache(maxsize=64)
def schedule(n, ndom, must, groups=1, seed=0, cg=0, launches=0):
    """(launches, ndom) int64: the hot position of every domain in every launch.  ``must``: tuple of (group, position) -- bound
    to the domains of that group (domain d belongs to group d % groups) --, (-1, position) -- any domain --, or (-2, pixel) -- any
    domain and any channel of the pixel (``must_hit`` when the channels had to be thinned).  Bound entries take the first slots
    of their group's domains.  Without ``cg`` the others are dealt to the remaining slots in (launch, domain) order.  With
    ``cg`` (positions are pixel * cg + channel) every domain WANTS a channel for each of its free slots in turn -- a cycle that
    starts at the group's index, with the images of a batch spread over it -- so that every channel of every group comes up: dealt straight, position p would always land in domain
    p mod ndom, and with ndom a multiple of the groups a workgroup owns, a channel's place in its group and the group's place
    in its workgroup would share their residue -- half the channels of a slice would never be hot.  A slot takes the next
    listed position with the wanted channel, else the next (-2) pixel at the wanted channel; positions left over take the
    slots still free; a seeded pixel at the wanted channel (without ``cg``: a seeded position) fills the rest.  At least
    ``launches`` launches.  Raises if BUDGET launches cannot hold ``must``; that every (group, channel) is hot is asserted by
    test_stat_probe_cpu.py for every case."""
    bound = [e for e in must if e[0] >= 0]
    listed = [p for g, p in must if g == -1]
    pixels = [p for g, p in must if g == -2]
    per = ndom // groups
    need = max([0] + [-(-sum(1 for e in bound if e[0] == g) // per) for g in {e[0] for e in bound}])
    launches = max(1, launches, need, -(-len(must) // ndom))
    assert launches <= BUDGET, f"{len(must)} must-hit positions do not fit {BUDGET} launches of {ndom} domains"
    slots = torch.full((launches, ndom), -1, dtype=torch.int64).tolist()
    taken = {}
    for g, p in bound:
        k = taken.get(g, 0)                                  # k-th slot of group g: launch-major over its domains
        slots[k // per][(k % per) * groups + g] = p
        taken[g] = k + 1
    gen = torch.Generator().manual_seed(0xD0 + 131 * seed + n + 7 * ndom)
    holes = [(l, d) for l in range(launches) for d in range(ndom) if slots[l][d] < 0]
    rnd = torch.randint(0, n // cg if cg else n, (len(holes),), generator=gen).tolist()
    if not cg:
        for i, (l, d) in enumerate(holes):
            slots[l][d] = listed[i] if i < len(listed) else rnd[i]
        return torch.tensor(slots)
    buckets = [[p for p in listed if p % cg == c][::-1] for c in range(cg)]
    pixels = pixels[::-1]
    # a domain's wanted channels in turn: those its group's bound entries do not bring first, images spread over the cycle
    mine = {g: {p % cg for gg, p in bound if gg == g} for g in {e[0] for e in bound}}
    spread = -(-cg // per)
    cycle = []
    for d in range(ndom):
        rot = [(i + (d // groups) * spread + d % groups) % cg for i in range(cg)]
        got = mine.get(d % groups, ())
        cycle.append([c for c in rot if c not in got] + [c for c in rot if c in got])
    count, want, later = [0] * ndom, {}, []
    for l, d in holes:
        c = want[l, d] = cycle[d][count[d] % cg]
        count[d] += 1
        if buckets[c]:
            slots[l][d] = buckets[c].pop()
        elif pixels:
            slots[l][d] = pixels.pop() * cg + c
        else:
            later.append((l, d))
    left = [p for bk in buckets for p in bk[::-1]]
    assert len(left) <= len(later), f"{len(must)} must-hit positions do not fit {launches} launches of {ndom} domains"
    for i, (l, d) in enumerate(later):
        slots[l][d] = left[i] if i < len(left) else rnd[i] * cg + want[l, d]
    return torch.tensor(slots)


def covered(slots, must, groups=1, cg=0):
    """does the schedule make every entry of ``must`` hot -- in a domain of its group where it names one, at any channel of the
    pixel where it names a pixel (-2; needs ``cg``)?"""
    flat = slots.reshape(-1).tolist()
    have_any, have_px = set(flat), {p // cg for p in flat} if cg else set()
    dom_group = (torch.arange(slots.shape[1]) % groups).expand_as(slots).reshape(-1).tolist()
    have = set(zip(dom_group, flat))
    return all((p in have_px) if g == -2 else (p in have_any) if g == -1 else ((g, p) in have) for g, p in must)


# ------------------------------------------------------------------------------------------------ references (fp64)
def _affine(y, gam, bet):
    if gam is None:
        return y
    d, n = y.shape
    return (y.reshape(-1, gam.shape[0], n) * gam.to(y.device) + bet.to(y.device)).reshape(d, n)


def reference(x, eps=1e-5, gam=None, bet=None, silu=False, scale=1.0):
    """plain normalisation of every row of the domain-major x in fp64: (x - mean) / sqrt(var + eps) with the biased variance,
    times the (groups, n) factor, plus the offset, SiLU, a constant factor (the GEGLU forms: gelu of the constant gate)"""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = _affine((x - mean) / torch.sqrt(var + eps), gam, bet)
    if silu:
        y = y * torch.sigmoid(y)
    return y * scale


def refnorm_reference(x):
    """test_refnorm's reference on the domain-major view, in fp64: unbiased std, clamp at 1e-6, times 0.5"""
    x = x.double()
    r = x - x.mean(1, keepdim=True)
    return r / torch.clamp(r.std(1, unbiased=True, keepdim=True), min=1e-6) * 0.5


# ------------------------------------------------------------------------------------------------ the check
def check(got, want, hot, lay, what="", hot_tol=TOL):
    """Two tiers per domain on domain-major tensors (any device); returns (worst hot error, worst other error), each as a
    fraction of its limit.  The message of a failure names the domain, the hot position and the tier."""
    got, want = got.double(), want.double().to(got.device)
    hot = hot.to(got.device)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    col = hot[:, None]
    err = (got - want).abs()
    hot_err, hot_lim = err.gather(1, col)[:, 0], hot_tol * want.gather(1, col)[:, 0].abs()
    err = err.scatter(1, col, 0.0)
    rest_err, rest_at = err.max(1)
    rest_lim = TOL * want.abs().scatter(1, col, 0.0).amax(1) + FLOOR
    bad_hot, bad_rest = hot_err > hot_lim, rest_err > rest_lim
    if bool(bad_hot.any()) or bool(bad_rest.any()):
        tier, bad = ("hot", bad_hot) if bool(bad_hot.any()) else ("non-hot", bad_rest)
        d = int(bad.nonzero()[0])
        p = int(hot[d])
        at = p if tier == "hot" else int(rest_at[d])
        e, lim = (hot_err, hot_lim) if tier == "hot" else (rest_err, rest_lim)
        raise AssertionError(f"{what}: {tier} tier fails in {int(bad.sum())} of {len(bad)} domains; first: domain {d}, hot at "
                             f"{lay.where(d, p)}; output at {lay.where(d, at)}: got {float(got[d, at]):.6g}, want "
                             f"{float(want[d, at]):.6g}, |err| {float(e[d]):.4g} > limit {float(lim[d]):.4g}")
    return float((hot_err / hot_lim).max()), float((rest_err / rest_lim).max())


def passes(got, want, hot, lay, hot_tol=TOL):
    try:
        return check(got, want, hot, lay, hot_tol=hot_tol)
    except AssertionError:
        return None


# ------------------------------------------------------------------------------------------------ fp32 emulation with faults
def emulate(x, hot, fault=None, eps=1e-5, gam=None, bet=None, silu=False, scale=1.0, groups=1, refnorm=False):
    """The operation in torch fp32 on the domain-major bf16 x, output rounded to bf16 -- with one of FAULTS applied to the
    element at hot[d] of every domain: ``drop`` leaves it out of both sums, ``twice`` counts it twice in both, ``novar`` leaves
    it out of the sum of squared deviations only, ``neighbour`` books it to the next group of the same image (GroupNorm:
    ``groups`` domains per image) or to the next row -- in every second domain only: all domains carry the same V, so a move
    in every one of them would cancel, and a kernel's fault sits at fixed positions, which are hot in few domains of a launch.
    The divisor stays N."""
    x = x.float()
    d, n = x.shape
    col = hot[:, None].to(x.device)
    h = x.gather(1, col)
    moved = h * (torch.arange(d, device=x.device)[:, None] % 2 == 0) if fault == "neighbour" else None
    nb = lambda t: t.reshape(-1, groups, 1).roll(1, 1).reshape(d, 1) if groups > 1 else t.roll(1, 0)   # noqa: E731
    s = x.sum(1, keepdim=True)
    if fault == "drop":
        s = s - h
    if fault == "twice":
        s = s + h
    if fault == "neighbour":
        s = s - moved + nb(moved)
    mean = s / n
    q = ((x - mean) ** 2).sum(1, keepdim=True)
    if fault in ("drop", "novar"):
        q = q - (h - mean) ** 2
    if fault == "twice":
        q = q + (h - mean) ** 2
    if fault == "neighbour":
        gone, come = moved != 0, nb(moved) != 0
        q = q - gone * (h - mean) ** 2 + come * (nb(moved) - mean) ** 2
    if refnorm:
        y = (x - mean) * (0.5 / torch.clamp(torch.sqrt(q / (n - 1)), min=1e-6))
    else:
        y = (x - mean) * torch.rsqrt(q / n + eps)
        if gam is not None:
            y = _affine(y, gam.float(), bet.float())
        if silu:
            y = y * torch.sigmoid(y)
        y = y * scale
    return y.to(torch.bfloat16)


def gelu64(c):
    return 0.5 * c * (1.0 + math.erf(c / math.sqrt(2.0)))
