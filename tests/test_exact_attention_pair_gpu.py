"""Bit-exact tests of attention launches with TWO problems (MvdAttnArgs::nprob = 2), the form every transformer block of an
image-conditioned forward issues twice: self-attention with the adapter's reference attention, text cross-attention with the
reference cross-attention.  ``ops.attention_pair`` (mvd_debug_attention_pair) fills one MvdAttnArgs with two problems and calls
mvd_launch_attention -- what the engine does; every other operator entry launches one problem.

What a two-problem launch adds to the kernel: the workgroup id is decoded over heads * batch * 2 (* ranges) pairs, in the
XCD-swizzled branch or the plain one; the problem index selects nq, nk, every pointer and stride and the K/V map; the split-KV
workspace, its (pair, query block) counters and the merge run over both problems.  The routing data (exact_util.routing_pair,
tests/pair_util.py) give every K/V element of both problems values of its own, so a row answered from the other problem's K, V,
key count, map or workspace slot, or by a neighbouring pair, has other bits (tests/test_attention_pair_cpu.py shows each on the
data).  Every comparison is exact_util.assert_same_bits; no case has a tolerance.

(a) unsplit routing, (b) split-KV routing, (c) the four map combinations of the shared forwards, (d) on Gaussian data a pair equals
its two single-problem launches bit for bit, (e) the split the engine itself picks at the batch-1 64x64 level, (f) rejections."""
import contextlib

import pytest
import torch

import exact_util as X
import pair_util as P

pytestmark = pytest.mark.gpu

GAINS = (X.LAZY, X.STRICT_LAZY, X.RERUN)
FILL = 7.0          # no routing output: |v| < 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


@contextlib.contextmanager
def forced_waves(nw_log2):
    from mvd_amd import _lib as L
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        yield
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


def _full(*shape):
    return torch.full(shape, FILL, dtype=torch.bfloat16, device="cuda")


def operands(d, fused):
    """-> the two problem dicts of ops.attention_pair, outputs pre-filled, and a check that everything around the outputs still holds
    the fill.  Contiguous operands, or -- ``fused`` -- the engine's layout: both problems' queries are column ranges of ONE buffer with
    row stride 4 C ([q0 | . | . | q1], as qkv and qkv + 3 C), problem 0's K/V column ranges of rows of 3 C, problem 1's of rows of
    4 C ([k | v | . | .], the reference K/V), both outputs column ranges of one buffer of 3 C; the fill in between.  The buffers have
    max(nq0, nq1) rows: problem 1's workgroups past its own queries must leave without writing."""
    C, B = d.heads * 64, d.B
    p0, p1 = d.prob
    assert B == 1 or p0.nq == p1.nq           # (batch strides are n * ld)
    rows = max(p0.nq, p1.nq)
    if not fused:
        outs = [_full(B, rows, C), _full(B, rows, C)]
        args = [dict(q=p.q.cuda(), k=p.k.cuda(), v=p.v.cuda(), out=o[:, :p.nq], **p.map) for p, o in zip(d.prob, outs)]
        return args[0], args[1], lambda: all(bool((o[:, p.nq:] == FILL).all()) for p, o in zip(d.prob, outs))
    qb, ob = _full(B, rows, 4 * C), _full(B, rows, 3 * C)
    kv0, kv1 = _full(p0.k.shape[0], p0.nk, 3 * C), _full(p1.k.shape[0], p1.nk, 4 * C)
    qb[:, :p0.nq, :C], qb[:, :p1.nq, 3 * C:] = p0.q.cuda(), p1.q.cuda()
    kv0[:, :, C:2 * C], kv0[:, :, 2 * C:] = p0.k.cuda(), p0.v.cuda()
    kv1[:, :, :C], kv1[:, :, C:2 * C] = p1.k.cuda(), p1.v.cuda()
    a0 = dict(q=qb[:, :p0.nq, :C], k=kv0[:, :, C:2 * C], v=kv0[:, :, 2 * C:], out=ob[:, :p0.nq, :C], **p0.map)
    a1 = dict(q=qb[:, :p1.nq, 3 * C:], k=kv1[:, :, :C], v=kv1[:, :, C:2 * C], out=ob[:, :p1.nq, 2 * C:], **p1.map)

    def untouched():
        return bool((ob[:, :, C:2 * C] == FILL).all() and (ob[:, p0.nq:, :C] == FILL).all() and (ob[:, p1.nq:, 2 * C:] == FILL).all())
    return a0, a1, untouched


def workgroups(d, waves, nsplit=1):
    qb = 32 * waves
    return (max(p.nq for p in d.prob) + qb - 1) // qb * d.heads * d.B * 2 * nsplit


def check_pair(ops, d, fused, waves, what, ws="own"):
    a0, a1, untouched = operands(d, fused)
    o0, o1 = ops.attention_pair(a0, a1, d.heads, scale=d.scale, nsplit=d.nsplit, ws=ws)
    plan = ops.last_attention_plan()
    assert plan == dict(waves=waves, workgroups=workgroups(d, waves, d.nsplit)), (plan, what)
    X.assert_same_bits(o0, d.prob[0].want, f"{what}, problem 0")
    X.assert_same_bits(o1, d.prob[1].want, f"{what}, problem 1")
    assert untouched(), f"{what}: written outside the outputs"


# ------------------------------------------------------------------------------------------------ (a) routing, unsplit
@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", P.ROUTE)
def test_pair_routes_exactly(ops, case, prescaled, nw_log2):
    """every wave-count form (forced, plan asserted), generic and engine softmax, the three gain regimes, contiguous operands and the
    engine's fused layout; rows past a problem's queries and the columns between the outputs keep their fill"""
    with forced_waves(nw_log2):
        for gain in GAINS:
            d = P.build(P.route_case(case), gain, prescaled)
            for fused in (False, True):
                check_pair(ops, d, fused, 1 << nw_log2, f"pair {case} prescaled {prescaled} waves {1 << nw_log2} gain {gain} fused {fused}")


# ------------------------------------------------------------------------------------------------ (b) routing, split-KV
def check_split(ops, d, what):
    """twice in a row on one workspace -- a counter the first run left non-zero, or a partial it left behind, would show in the second
    -- and once on a workspace full of NaN patterns, which a merge that reads a slot nobody wrote would return"""
    for fused in (False, True):
        a0, a1, _ = operands(d, fused)
        ws = ops.attention_pair_ws(a0, a1, d.heads, d.scale, d.nsplit)
        assert ws is not None
        for run in ("first run", "second run on the same workspace"):
            check_pair(ops, d, fused, 4, f"{what} fused {fused}, {run}", ws)
        ws.fill_(0xFF)
        check_pair(ops, d, fused, 4, f"{what} fused {fused}, workspace of NaNs", ws)


@pytest.mark.parametrize("case", P.SPLIT)
def test_pair_split_routes_exactly(ops, case):
    """the chosen keys lie on both sides of every range boundary of their own problem (must_hit(nk_i, nsplit))"""
    for gain in GAINS:
        check_split(ops, P.build(P.split_case(case), gain, True), f"split pair {case} gain {gain}")


# ------------------------------------------------------------------------------------------------ (c) maps that differ
@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", P.MAPPED, ids=[c[0] for c in P.MAPPED])
def test_pair_with_two_maps_routes_exactly(ops, case, prescaled, nw_log2):
    """the four map combinations the engine issues (pair_util.layout): none | group, group | group, group | group x objects,
    table | table -- problem 0 the text K/V, problem 1 the reference K/V"""
    with forced_waves(nw_log2):
        for gain in GAINS:
            d = P.build(P.mapped_case(case), gain, prescaled)
            for fused in (False, True):
                check_pair(ops, d, fused, 1 << nw_log2, f"pair {case} prescaled {prescaled} waves {1 << nw_log2} gain {gain} fused {fused}")


def test_pair_with_a_group_and_a_split_routes_exactly(ops):
    """the launcher accepts a group together with a split: the base pointers alone change"""
    for gain in GAINS:
        check_split(ops, P.build(P.mapped_case(P.MAPPED_SPLIT), gain, True), f"split pair {P.MAPPED_SPLIT} gain {gain}")


# ------------------------------------------------------------------------------------------------ (d) a pair is its two halves
def gaussian(case, seed=0):
    """seeded Gaussian q (B, nq, C) and k, v (E, nk, C) per problem of a case: all 64 keys of a tile weigh"""
    name, B, heads, nq0, nk0, nq1, nk1, _ = case
    B, lay = P.layout(name, B)
    gen = torch.Generator().manual_seed(100 + seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)      # noqa: E731
    return B, [dict(q=rnd(B, nq, heads * 64).cuda(), k=rnd(E, nk, heads * 64).cuda(), v=rnd(E, nk, heads * 64).cuda(), **kw)
               for (E, _, kw, _, _), nq, nk in zip(lay, (nq0, nq1), (nk0, nk1))]


def single(ops, p, heads, scale, nsplit):
    """the single-problem operator entry of the same map"""
    q, k, v = p["q"], p["k"], p["v"]
    if nsplit > 1:
        assert scale == 0.0 and len(p) == 3
        return ops.attention_split(q, k, v, heads, nsplit)
    if "kv_index" in p:
        return ops.attention_mapped(q, k, v, heads, p["kv_index"], scale=scale)
    if "kv_objects" in p:
        return ops.attention_objects(q, k, v, heads, p["kv_group"], p["kv_objects"], scale=scale)
    if "kv_group" in p:
        return ops.attention_grouped(q, k, v, heads, p["kv_group"], scale=scale)
    return ops.attention(q, k, v, heads, scale=scale)


def check_halves(ops, probs, heads, scale, nsplit, what):
    o0, o1 = ops.attention_pair(probs[0], probs[1], heads, scale=scale, nsplit=nsplit)
    for i, (got, p) in enumerate(zip((o0, o1), probs)):
        X.assert_same_bits(got, single(ops, p, heads, scale, nsplit).cpu(), f"{what}: problem {i} of the pair against its own launch")
    assert not torch.equal(o0[:, :32], o1[:, :32])


HALVES = [P.route_case(P.ROUTE[0]), P.route_case(P.ROUTE[1]), P.route_case(P.ROUTE[5]), P.mapped_case(P.MAPPED[0]), P.mapped_case(P.MAPPED[2]),
          P.mapped_case(P.MAPPED[3])]


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("case", HALVES, ids=str)
def test_pair_equals_its_two_launches(ops, case, nw_log2):
    """a workgroup's arithmetic depends on its own problem alone: both outputs of a pair launch are those of two single-problem
    launches at the same forced wave count, both softmax forms"""
    _, probs = gaussian(case)
    with forced_waves(nw_log2):
        for scale in (0.125, 0.0):
            check_halves(ops, probs, case[2], scale, 1, f"{case} waves {1 << nw_log2} scale {scale}")


@pytest.mark.parametrize("case", [P.split_case(c) for c in P.SPLIT], ids=str)
def test_split_pair_equals_its_two_launches(ops, case):
    """... and the merge adds the ranges in index order whoever arrives last: the same bits as two split launches of one problem"""
    _, probs = gaussian(case, 1)
    check_halves(ops, probs, case[2], 0.0, case[7], f"{case}")


@pytest.mark.parametrize("nsplit,victim", [(1, 0), (1, 1), (2, 1)])
def test_pair_with_the_fallback_in_one_problem_equals_its_two_launches(ops, nsplit, victim):
    """the running-max fallback in ONE problem only (test_ops_gpu.py test_attention_running_max_fallback: the scores of the keys from
    ``jump`` on lie ~190 above the earlier ones for half the queries, the engine form's denominators overflow and the workgroup
    re-runs its tiles checked); the other problem's workgroups keep their unchecked result"""
    B, heads, nq, nks, jump = 1, 2, 200, (320, 192), 130
    gen = torch.Generator().manual_seed(5 + victim)
    probs = []
    for i, nk in enumerate(nks):
        q, k = 0.05 * torch.randn(B, nq, heads * 64, generator=gen), 0.05 * torch.randn(B, nk, heads * 64, generator=gen)
        v = torch.randn(B, nk, heads * 64, generator=gen)
        if i == victim:
            q[:, :nq // 2] += 1.0
            k[:, :jump] -= 1.5
            k[:, jump:] += 1.5
        probs.append(dict(q=q.to(torch.bfloat16).cuda(), k=k.to(torch.bfloat16).cuda(), v=v.to(torch.bfloat16).cuda()))
    with forced_waves(2):
        check_halves(ops, probs, heads, 0.0, nsplit, f"fallback in problem {victim}, nsplit {nsplit}")
    for p in probs:
        assert bool(torch.isfinite(single(ops, p, heads, 0.0, nsplit).float()).all())


# ------------------------------------------------------------------------------------------------ (e) the production split
def test_engines_own_split_at_the_batch_1_64x64_level(ops):
    """nsplit = 0 is mvd_attention_pick_split on the launch's own arguments: two problems of 4096 queries and keys, 5 heads,
    batch 1 -- 1280 waves, so the heuristic cuts the keys of BOTH problems in two: 32 query blocks x 5 heads x 2 problems x 2
    ranges = 640 workgroups of 4 waves.  The outputs are those of two ops.attention_split(nsplit=2) launches."""
    from mvd_amd.packing import QSCALE
    heads, n = 5, 4096
    gen = torch.Generator().manual_seed(64)
    rnd = lambda s=1.0: (torch.randn(1, n, heads * 64, generator=gen) * s).to(torch.bfloat16).cuda()      # noqa: E731
    probs = [dict(q=rnd(QSCALE), k=rnd(), v=rnd()) for _ in range(2)]
    o0, o1 = ops.attention_pair(probs[0], probs[1], heads, scale=0.0, nsplit=0)
    assert ops.last_attention_plan() == dict(waves=4, workgroups=640)
    for i, (got, p) in enumerate(zip((o0, o1), probs)):
        X.assert_same_bits(got, ops.attention_split(p["q"], p["k"], p["v"], heads, 2).cpu(), f"problem {i} against attention_split(nsplit=2)")


# ------------------------------------------------------------------------------------------------ (f) rejections
def _zeros(B, n):
    return torch.zeros(B, n, 64, dtype=torch.bfloat16, device="cuda")


@pytest.mark.parametrize("name,nk0,nk1,scale,nsplit,ws,map1,msg", [
    ("nine ranges", 1024, 1024, 0.0, 9, "own", {}, "bad split-KV request (nsplit=9"),
    ("a split with the generic softmax", 128, 128, 0.125, 2, "own", {}, "bad split-KV request (nsplit=2"),
    ("problem 1 alone too short for the split", 256, 127, 0.0, 2, "own", {}, "bad split-KV request (nsplit=2, fewest keys 127)"),
    ("a table with a group on problem 1", 128, 128, 0.0, 1, "own", dict(kv_index=[0, 1, 2, 3, 0, 0], kv_group=2),
     "problem 1 sets a K/V table together with K/V group 2"),
    ("a table entry outside problem 1's elements", 128, 128, 0.0, 1, "own", dict(kv_index=[0, 1, 2, 3, 4, 0]), "entry 4 is 4, outside the 4 K/V elements"),
    ("a null workspace with a split", 128, 128, 0.0, 2, None, {}, "bad split-KV request (nsplit=2"),
])
def test_pair_rejections_launch_nothing(ops, name, nk0, nk1, scale, nsplit, ws, map1, msg):
    """each returns non-zero with the launcher's message, leaves both pre-filled outputs as they were and the thread's launch plan
    what the launch before made it"""
    from mvd_amd import _lib as L
    B, nq = 6, 33
    with forced_waves(0):
        ops.attention_pair(dict(q=_zeros(B, nq), k=_zeros(B, 63), v=_zeros(B, 63)), dict(q=_zeros(B, nq), k=_zeros(B, 65), v=_zeros(B, 65)), 1)
    before = ops.last_attention_plan()
    assert before == dict(waves=1, workgroups=2 * B * 2)
    E1 = 4 if "kv_index" in map1 else B
    outs = [_full(B, nq, 64), _full(B, nq, 64)]
    p0 = dict(q=_zeros(B, nq), k=_zeros(B, nk0), v=_zeros(B, nk0), out=outs[0])
    p1 = dict(q=_zeros(B, nq), k=_zeros(E1, nk1), v=_zeros(E1, nk1), out=outs[1], **map1)
    with forced_waves(2):                     # an accepted launch would now record another plan
        rc, _, _ = ops.attention_pair(p0, p1, 1, scale=scale, nsplit=nsplit, ws=ws, check=False)
    assert rc != 0 and msg in L.last_error(), (name, rc, L.last_error())
    torch.cuda.synchronize()
    assert all(bool((o == FILL).all()) for o in outs) and ops.last_attention_plan() == before, name
