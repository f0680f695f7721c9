"""The spike probes keep their promise, and the gap they close is real -- all on the CPU (counterpart of test_exact_inputs_cpu.py).

For every case of test_stat_probe_gpu.py (its case lists are imported; launch 0 of each), on a torch fp32 emulation of the
operation with bf16 output:

(a) the fault-free emulation passes the two-tier check with margin (at most 3/4 of either limit);
(b) dropping the hot element, counting it twice, leaving it out of the variance only, and booking it to the neighbouring group
    (GroupNorm) or row each fail it;
(c) the same four faults on the Gaussian inputs of test_ops_gpu.py's test_groupnorm / test_layernorm PASS that file's ``close``
    where N is large against one element -- GroupNorm and the 1280-wide LayerNorm rows: on a seeded element of every domain.  A row
    of 320 is short enough for ``close`` to see the fault on one of its largest elements (9 sigma^2 of 320 sigma^2); there the
    faults pass on the element of median size of every row.  That is the gap: not every fault, but most elements of every
    domain.

Also: the must-hit builder covers what it claims for hand-written plans, the schedules hold their must-hit lists, and the
exhaustive cases are exhaustive."""
import os

import pytest
import torch
import torch.nn.functional as F

import stat_probe as P
import test_stat_probe_gpu as T
from test_ops_gpu import close, rnd

MARGIN = 0.75


def _abc(lay, x, hot, want, what, hot_tol=P.TOL, **emu):
    ok = P.check(P.emulate(x, hot, None, **emu), want, hot, lay, what, hot_tol)
    assert max(ok) <= MARGIN, (what, ok)
    for fault in P.FAULTS:
        assert P.passes(P.emulate(x, hot, fault, **emu), want, hot, lay, hot_tol) is None, f"{what}: '{fault}' goes unseen"
    return ok


# ------------------------------------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case", T.GN_SLICE_CASES + T.GN_TWO_CASES, ids=T.case_id)
def test_groupnorm_probe_sees_the_faults(case, silu):
    name, B, hw, c0, c1, shift, flag, plan = case
    lay, must, info, slots = T.gn_probe(case)
    assert len(slots) <= P.BUDGET and P.covered(slots, must, T.GROUPS, lay.cg)
    if lay.n <= P.EXHAUSTIVE_MAX:
        assert set(slots.reshape(-1).tolist()) == set(range(lay.n)), "not exhaustive"
    else:
        assert len(slots) >= T.FILL_LAUNCHES
    # every channel of the tensor is hot somewhere -- every (group, channel in group), hence every place a channel can have in a
    # workgroup's slice and either side of every group boundary inside a thread's vector
    grp = (torch.arange(lay.ndom) % T.GROUPS).expand_as(slots).reshape(-1)
    pos = slots.reshape(-1)
    assert len(set(zip(grp.tolist(), (pos % lay.cg).tolist()))) == T.GROUPS * lay.cg, "a channel is never hot"
    gpw = plan.get("gpw", 1)
    assert len(set(zip((grp % gpw).tolist(), (pos % lay.cg).tolist()))) == gpw * lay.cg
    gam, bet = lay.affine(*T.gn_affine(c0 + c1))
    x = P.with_spike(P.background(lay.ndom, lay.n, hw + c0, shift), slots[0])
    _abc(lay, x, slots[0], P.reference(x, 1e-5, gam, bet, silu), f"groupnorm {name}", gam=gam, bet=bet, silu=silu, groups=T.GROUPS)


@pytest.mark.parametrize("c", T.LN_C)
def test_layernorm_probe_sees_the_faults(c):
    rows = c + 3
    lay, hot = P.Rows(rows, c), T.ln_hot(rows, c)
    assert set(hot.tolist()) == set(range(c)), "not exhaustive"
    gam, bet = lay.affine(*T.ln_affine(c))
    x = P.with_spike(P.background(rows, c, c), hot)
    _abc(lay, x, hot, P.reference(x, 1e-5, gam, bet), f"layernorm {c}", gam=gam, bet=bet)


@pytest.mark.parametrize("case", T.REFNORM_CASES, ids=T.case_id)
def test_refnorm_probe_sees_the_faults(case):
    lay, slots = T.refnorm_probe(case)
    assert len(slots) <= P.BUDGET and set(slots.reshape(-1).tolist()) == set(range(lay.n)), "not exhaustive"
    x = P.with_spike(P.background(lay.ndom, lay.n, case[0]), slots[0])
    _abc(lay, x, slots[0], P.refnorm_reference(x), f"refnorm {case}", refnorm=True)


@pytest.mark.parametrize("case", T.FOLD_CASES, ids=T.case_id)
def test_fold_probe_sees_the_faults(case):
    kernel, k, m, geglu, cfg = case
    lay = P.Rows(m, k)
    hots = T.fold_slots(k, m)
    for col in range(k):                # every column hot in two rows of different 16-row MFMA tiles and of different lanes
        r = (hots == col).nonzero()[:, 1]
        assert len(set((r // 16).tolist())) >= 2 and len(set((r % 16).tolist())) >= 2, (case, col)
    gamma, beta = T.fold_affine(k)
    assert torch.equal(gamma, gamma.to(torch.bfloat16).float()) and torch.equal(beta, beta.to(torch.bfloat16).float())
    gam, bet = lay.affine(gamma, beta)
    scale = P.gelu64(T.GEGLU_GATE) if geglu else 1.0
    hot_tol = P.TOL + (P.GELU_ERR / abs(scale) if geglu else 0.0)
    x = P.with_spike(P.background(m, k, k + m), hots[0])
    _abc(lay, x, hots[0], P.reference(x, 1e-5, gam, bet, scale=scale), f"fold {case}", hot_tol, gam=gam, bet=bet, scale=scale)


# ------------------------------------------------------------------------------------------------ (c) the gap
@pytest.mark.parametrize("hw,C", [(64, 1280), (1024, 320), (4096, 320)])       # N = 2560, 10240, 40960
@pytest.mark.parametrize("fault", P.FAULTS)
def test_tolerance_test_misses_the_faults_groupnorm(hw, C, fault):
    """test_groupnorm's inputs and check: a GroupNorm that mistreats one element per group still passes ``close``."""
    B = 2
    x = (rnd(B, hw, C, seed=1, scale=2.0) + 0.5).to(torch.bfloat16)
    g, b = 1 + 0.1 * rnd(C, seed=3, dtype=torch.float32), 0.1 * rnd(C, seed=4, dtype=torch.float32)
    want = F.group_norm(x.float().permute(0, 2, 1), 32, g, b, 1e-5).permute(0, 2, 1)
    lay = P.GN(B, hw, C)
    hot = P.schedule(lay.n, lay.ndom, (), T.GROUPS, seed=hw)[0]
    gam, bet = lay.affine(g, b)
    got = lay.from_dom(P.emulate(lay.to_dom(x), hot, fault, gam=gam, bet=bet, groups=T.GROUPS))
    close(got, want, what=f"groupnorm with '{fault}'")


@pytest.mark.parametrize("rows,c", [(100, 320), (33, 1280)])
@pytest.mark.parametrize("fault", P.FAULTS)
def test_tolerance_test_misses_the_faults_layernorm(rows, c, fault):
    """test_layernorm's inputs and check; the mistreated element is a seeded one in the 1280-wide rows, the one of median size in
    the 320-wide rows (short enough for ``close`` to see the same fault on one of the largest elements)"""
    x = rnd(rows, c, seed=1, scale=3.0)
    g, b = 1 + 0.1 * rnd(c, seed=2, dtype=torch.float32), 0.1 * rnd(c, seed=3, dtype=torch.float32)
    lay = P.Rows(rows, c)
    gam, bet = lay.affine(g, b)
    hot = x.float().abs().argsort(1)[:, c // 2] if c == 320 else P.schedule(c, rows, (), 1, seed=c)[0]
    got = P.emulate(x, hot, fault, gam=gam, bet=bet)
    close(got, F.layer_norm(x.float(), (c,), g, b, 1e-5), what=f"layernorm with '{fault}'")


# ------------------------------------------------------------------------------------------------ the builder and the check
def test_must_hit_covers_what_it_claims():
    hw, cg = 50, 4
    every = lambda px: {(-1, q * cg + cc) for q in px for cc in range(cg)}      # noqa: E731
    # slice form, 16 pixels per pass: edges, and both sides of 16, 32, 48
    must, info = P.must_hit(dict(form="slice", npl=16), hw, cg)
    assert info["full"] and set(must) == every([0, 1, 48, 49, 15, 16, 31, 32, 47])
    # two-kernel form: chunks of 20 rows, 3 rows in flight, apply blocks of 7 rows; c0 = 10 lies inside group 2 (channels 8..11)
    plan = dict(form="two_kernel", R=3, rows_per_chunk=20, apply_rows=7)
    px = [0, 1, 48, 49, 19, 20, 39, 40, 2, 21, 22, 41, 42] + [q for t in range(7, 50, 7) for q in (t - 1, t)]
    must, info = P.must_hit(plan, hw, cg, c0=10)
    assert info["full"] and {e for e in must if e[0] < 0} == every(px)
    assert {e for e in must if e[0] >= 0} == {(2, q * cg + cc) for q in (0, 1, 48, 49, 19, 20) for cc in (1, 2)}
    # c0 on a group edge: the last channel of group 1 and the first of group 2
    must, _ = P.must_hit(plan, hw, cg, c0=8)
    assert {e for e in must if e[0] >= 0} == {(g, q * cg + cc) for q in (0, 1, 48, 49, 19, 20) for g, cc in ((1, 3), (2, 0))}
    # too little room for the cross product: every pixel once, its channel left to the schedule; less still: the tail goes
    upx = list(dict.fromkeys(px))
    must, info = P.must_hit(plan, hw, cg, capacity=2 * len(upx) + 1)
    assert not info["full"] and info["channels"] == 1 and list(must) == [(-2, q) for q in upx]
    must, info = P.must_hit(plan, hw, cg, c0=10, capacity=10)
    assert info["kept"] == 6 and list(must) == [(2, 1), (2, 2), (2, 49 * cg + 1), (2, 49 * cg + 2)] + [(-2, q) for q in upx[:6]]
    slots = P.schedule(hw * cg, 8, must, groups=4, seed=1, cg=cg)
    assert P.covered(slots, must, 4, cg) and not P.covered(slots * 0 + 3 * cg, must, 4, cg)
    # a schedule holds its list, bound entries in domains of their group, and is a pure function
    must, _ = P.must_hit(plan, hw, cg, c0=10)
    slots = P.schedule(hw * cg, 8, must, groups=4, seed=1, cg=cg)
    assert P.covered(slots, must, 4) and torch.equal(slots, P.schedule(hw * cg, 8, must, groups=4, seed=1, cg=cg))
    assert len(set(zip((torch.arange(8) % 4).expand_as(slots).reshape(-1).tolist(), (slots % cg).reshape(-1).tolist()))) == 4 * cg
    assert not P.covered(slots.roll(1, 1), must, 4)
    with pytest.raises(AssertionError):
        P.schedule(10 ** 6, 2, P.exhaustive(100), 1)


def test_spike_rule_and_check_messages():
    for n in (64, 320, 2560, 8192, 40960):
        v = P.spike(n)
        assert v * v >= 8 * n > (v / 2) ** 2 and v == 2.0 ** round(torch.log2(torch.tensor(v)).item())
    lay = P.GN(1, 4, 64, 32)
    want = torch.ones(32, 8, dtype=torch.float64)
    hot = torch.zeros(32, dtype=torch.int64)
    got = want.clone()
    got[5, 0] = 1.0 + 2 * P.TOL
    with pytest.raises(AssertionError, match=r"hot tier .* domain 5, hot at image 0, group 5, pixel 0, channel 10"):
        P.check(got, want, hot, lay, "x")
    got = want.clone()
    got[7, 3] = 1.0 + 2 * P.TOL
    with pytest.raises(AssertionError, match=r"non-hot tier .* domain 7, .* output at image 0, group 7, pixel 1, channel 15"):
        P.check(got, want, hot, lay, "x")
    got[7, 3] = 1.0 + P.TOL / 2
    assert P.check(got, want, hot, lay) == (0.0, pytest.approx(0.5, rel=1e-3))


def test_groupnorm_plan_hook_before_any_launch():
    """the C entry point refuses a null pointer and reports form 'none' on a thread that has launched nothing"""
    import threading
    from mvd_amd import _lib as L
    from mvd_amd import ops
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert L.lib().mvd_debug_last_groupnorm_plan(None) != 0 and "null" in L.last_error()
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.last_groupnorm_plan()))
    t.start()
    t.join()
    assert seen == [dict(form="none")]
