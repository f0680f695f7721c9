"""The data of tests/test_exact_attention_pair_gpu.py can see the faults a two-problem attention launch could have (the pattern of
test_objects_cpu.py and test_ragged_cpu.py: the fault is shown on the data, without a GPU).

For every routing case of the GPU file, exact_util.attention_reference -- fp64, rounded once to bf16 -- first returns the wanted
bits from the data as they are, and then, bent the way a faulty launch would bend it, other bits in at least one row of the problem
the fault touches:

* problem 1 answered from problem 0's K, and from problem 0's V (a per-problem pointer read at index 0);
* the longer problem's key count replaced by the shorter's (``nk`` read at index 0 or 1 for both; a count LONGER than a problem's
  own keys reads past them, which no reference emulates -- so the clamp to the shorter, and cases of equal counts have no such fault);
* problem 1's map replaced by problem 0's, where they differ (an element problem 1 does not have: its last);
* the two outputs exchanged;
* the pair decode off by one: every (problem, batch element, head) answered as its neighbour;
* split cases: one key range's partial of problem 1 taken from problem 0's workspace slot."""
import pytest
import torch

import exact_util as X
import pair_util as P

CASES = P.all_cases()
FORMS = [(c, pre) for c in CASES for pre in (False, True) if pre or c[7] == 1]      # (split-KV exists for the prescaled form only)
both_forms = pytest.mark.parametrize("case,prescaled", FORMS, ids=str)


def _data(case, prescaled):
    return P.build(case, X.LAZY, prescaled)


def _unit(d):
    return 1.0 if d.scale == 0.0 else d.scale * X.LOG2E


def _ref(d, q, k, v):
    return X.round_f64_to_bf16(X.attention_reference(q, k, v, d.heads, _unit(d)))


def _rows_changed(got, want):
    return int((got.view(torch.int16) != want.view(torch.int16)).any(-1).sum())


@both_forms
def test_reference_returns_the_wanted_bits(case, prescaled):
    d = _data(case, prescaled)
    for p in d.prob:
        X.assert_same_bits(_ref(d, p.q, p.k[p.table], p.v[p.table]), p.want, f"{case}")


@both_forms
def test_problem_1_from_problem_0s_operands_changes_rows(case, prescaled):
    d = _data(case, prescaled)
    p0, p1 = d.prob
    n = min(p0.nk, p1.nk)
    k0, v0, k1, v1 = p0.k[p0.table][:, :n], p0.v[p0.table][:, :n], p1.k[p1.table][:, :n], p1.v[p1.table][:, :n]
    assert _rows_changed(_ref(d, p1.q, k0, v1), p1.want) > 0, "K"
    assert _rows_changed(_ref(d, p1.q, k1, v0), p1.want) > 0, "V"


@pytest.mark.parametrize("case,prescaled", [f for f in FORMS if f[0][4] != f[0][6]], ids=str)
def test_the_other_problems_key_count_changes_rows(case, prescaled):
    d = _data(case, prescaled)
    n = min(p.nk for p in d.prob)
    p = max(d.prob, key=lambda p: p.nk)
    assert _rows_changed(_ref(d, p.q, p.k[p.table][:, :n], p.v[p.table][:, :n]), p.want) > 0


def test_key_counts_differ_in_most_cases():
    assert sum(c[4] != c[6] for c in CASES) >= len(CASES) - 1


@pytest.mark.parametrize("case,prescaled", [f for f in FORMS if f[0][0] not in ("plain", "views_cross")], ids=str)
def test_problem_0s_map_on_problem_1_changes_rows(case, prescaled):
    """views_self: no map against ``kv_group``; objects: ``kv_group`` against ``kv_group`` x ``kv_objects``; ragged: the text table against
    the adapter's.  (The cross form of the views layout gives both problems one map, the plain cases none.)"""
    d = _data(case, prescaled)
    p0, p1 = d.prob
    assert p0.table != p1.table and p0.map != p1.map
    wrong = [min(e, p1.k.shape[0] - 1) for e in p0.table]
    assert wrong != p1.table
    assert _rows_changed(_ref(d, p1.q, p1.k[wrong], p1.v[wrong]), p1.want) > 0


@both_forms
def test_exchanged_outputs_and_shifted_pairs_change_rows(case, prescaled):
    d = _data(case, prescaled)
    p0, p1 = d.prob
    n = min(p0.nq, p1.nq)
    assert _rows_changed(p0.want[:, :n], p1.want[:, :n]) > 0
    # the pair decode: pair = (problem * B + batch element) * heads + head; every pair answered as the next one
    blocks = [p.want[b, :, 64 * h:64 * (h + 1)] for p in d.prob for b in range(d.B) for h in range(d.heads)]
    assert len(blocks) == P.pairs(case) // d.nsplit
    for i, blk in enumerate(blocks):
        nxt = blocks[(i + 1) % len(blocks)]
        m = min(blk.shape[0], nxt.shape[0])
        assert _rows_changed(nxt[:m], blk[:m]) > 0, f"pair {i}"


def _partials(d, q, k, v, nk):
    """per key range of the split-KV kernel: (running max, denominator, normalised O) in fp64, each (B, heads, nq[, 64])"""
    B, nq, _ = q.shape
    sp = lambda t, n: t.double().reshape(B, n, d.heads, 64).transpose(1, 2)   # noqa: E731
    s = sp(q, nq) @ sp(k, nk).transpose(2, 3) * _unit(d)
    starts = X.split_starts(nk, d.nsplit) + [nk]
    out = []
    for a, b in zip(starts[:-1], starts[1:]):
        m = s[..., a:b].amax(-1)
        e = torch.exp2(s[..., a:b] - m[..., None])
        out.append((m, e.sum(-1), (e / e.sum(-1, keepdim=True)) @ sp(v, nk)[:, :, a:b]))
    return out


def _merge(d, parts):
    mmax = torch.stack([m for m, _, _ in parts]).amax(0)
    w = [l * torch.exp2(m - mmax) for m, l, _ in parts]
    o = sum(wi[..., None] * oi for wi, (_, _, oi) in zip(w, parts)) / sum(w)[..., None]
    B, _, nq, _ = o.shape
    return X.round_f64_to_bf16(o.transpose(1, 2).reshape(B, nq, d.heads * 64))


@pytest.mark.parametrize("case", [c for c in CASES if c[7] > 1], ids=str)
def test_a_partial_from_problem_0s_slot_changes_rows(case):
    d = _data(case, True)
    p0, p1 = d.prob
    parts = [_partials(d, p.q, p.k[p.table], p.v[p.table], p.nk) for p in d.prob]
    X.assert_same_bits(_merge(d, parts[1]), p1.want, "the merge of problem 1's own partials")
    n = min(p0.nq, p1.nq)
    for r in range(d.nsplit):
        bent = [tuple(t.clone() for t in part) for part in parts[1]]
        for own, other in zip(bent[r], parts[0][r]):
            own[:, :, :n] = other[:, :, :n]
        assert _rows_changed(_merge(d, bent), p1.want) > 0, f"range {r}"


def test_split_cases_meet_the_launchers_condition():
    split = [c for c in CASES if c[7] > 1]
    assert len(split) == len(P.SPLIT) + 1
    for c in split:
        assert min(c[4], c[6]) >= 64 * c[7], c
        # and in every (element, head) the chosen keys lie on both sides of every range boundary of their own problem
        B, lay = P.layout(c[0], c[1])
        (E0, m0, *_), (E1, m1, *_) = lay
        for p, nk in zip(X.routing_pair(E0, E1, c[2], m0 * c[3], c[4], m1 * c[5], c[6], X.LAZY, True, c[7]), (c[4], c[6])):
            edges = {k for s in X.split_starts(nk, c[7])[1:] for k in (s - 1, s)}
            assert edges and edges <= set(X.must_hit(nk, c[7]))
            for e in range(p.pi.shape[0]):
                for h in range(c[2]):
                    assert edges | {0, nk - 1} <= set(p.pi[e, h].tolist()), (c, e, h)


def test_cases_visit_both_decode_branches_unsplit_and_split():
    for split in (False, True):
        branches = {P.pairs(c) % 8 == 0 for c in CASES if (c[7] > 1) == split}
        assert branches == {True, False}, (split, branches)
    for cs in (P.ROUTE, P.MAPPED):
        assert {P.pairs(c) % 8 == 0 for c in map(P.route_case if cs is P.ROUTE else P.mapped_case, cs)} == {True, False}
