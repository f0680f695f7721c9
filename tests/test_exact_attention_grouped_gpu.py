"""Bit-exact tests of grouped K/V attention (``ops.attention_grouped``: batch element b attends the K/V of element b // kv_group --
V views of one object sharing its reference tokens).

The routing problem of exact_util.py for G objects with V * nq queries each IS the grouped problem: its q and want, viewed as
(G * V, nq, C) -- the same memory -- are V views of nq queries per object, and its k / v (G, nk, C) are what each object's views
share.  The correct output is v[b // V][pi], bit for bit: a view that reads another object's K/V (the ungrouped addressing, or a
group off by one) returns that object's V rows, whose values are hashed from the batch index and differ.  Every wave-count form
(1 / 2 / 4 waves, forced, plan asserted), generic and engine (prescaled) softmax, the three gain regimes of
test_exact_attention_gpu.py, contiguous operands and views of fused buffers."""
import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

# G, V, heads, nq, nk: (G, V) in {(1, 3), (2, 3), (2, 4)}, nq in {33, 144}, nk in {63, 65, 129, 1024}, heads 1 / 2 / 5 -- each value with
# each wave count and both softmax forms
CASES = [(1, 3, 1, 33, 63), (2, 3, 2, 144, 65), (2, 4, 5, 33, 129), (1, 3, 2, 144, 1024), (2, 4, 1, 144, 63), (2, 3, 5, 33, 1024),
         (1, 3, 5, 144, 129), (2, 4, 2, 33, 65)]
GAINS = (X.LAZY, X.STRICT_LAZY, X.RERUN)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def grouped_views(p, V):
    """(q (G V, nq, C), k, v (G, nk, C), want (G V, nq, C)) of the routing problem p over G objects with V * nq queries each"""
    G, n, C = p.q.shape
    return p.q.reshape(G * V, n // V, C), p.k, p.v, p.want.reshape(G * V, n // V, C)


def fused(q, k, v, junk=3.0):
    """q and k / v as column ranges of wider rows (row stride 3 C, as in fused projection outputs), junk in between"""
    B, nq, C = q.shape
    G, nk, _ = k.shape
    qb = torch.full((B, nq, 3 * C), junk, dtype=torch.bfloat16, device="cuda")
    kb = torch.full((G, nk, 3 * C), junk, dtype=torch.bfloat16, device="cuda")
    qb[:, :, :C] = q.cuda()
    kb[:, :, C:2 * C] = k.cuda()
    kb[:, :, 2 * C:] = v.cuda()
    return qb[:, :, :C], kb[:, :, C:2 * C], kb[:, :, 2 * C:]


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_grouped_attention_routes_exactly(ops, case, prescaled, nw_log2):
    from mvd_amd import _lib as L
    G, V, heads, nq, nk = case
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for gain in GAINS:
            p = X.routing_problem(G, heads, V * nq, nk, gain, prescaled)
            q, k, v, want = grouped_views(p, V)
            for what, (q_, k_, v_) in (("contiguous", (q.cuda(), k.cuda(), v.cuda())), ("fused views", fused(q, k, v))):
                got = ops.attention_grouped(q_, k_, v_, heads, kv_group=V, scale=p.scale)
                plan = ops.last_attention_plan()
                assert plan["waves"] == 1 << nw_log2, plan
                X.assert_same_bits(got, want, f"grouped attention {case} prescaled {prescaled} waves {1 << nw_log2} gain {gain} {what}")
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


def test_grouped_problem_tells_the_objects_apart():
    """the check above can see a wrong group: object 1's views answered from object 0's K/V differ (V is hashed from the batch)"""
    p = X.routing_problem(2, 2, 3 * 33, 65, X.LAZY, True)
    assert not torch.equal(p.v[0], p.v[1])
    _, _, _, want = grouped_views(p, 3)
    other = X.routing_values(2, 2, 65)[0].reshape(65, 2, 64)          # object 0's values at object 1's chosen keys
    wrong = other.permute(1, 0, 2)[torch.arange(2)[:, None], p.pi[1]].permute(1, 0, 2).reshape(3, 33, 128)
    assert not torch.equal(X.bf(wrong), want[3:])


@pytest.mark.parametrize("nw_log2", [-1, 0, 1, 2])
def test_group_of_one_is_plain_attention(ops, nw_log2):
    """kv_group = 1 (and the grouped launch against K/V repeated per view) is bit-identical to ops.attention on generic data"""
    from mvd_amd import _lib as L
    g = torch.Generator().manual_seed(14)
    B, V, heads, nq, nk = 6, 3, 2, 144, 129
    q = torch.randn(B, nq, heads * 64, generator=g).to(torch.bfloat16).cuda()
    k = torch.randn(B // V, nk, heads * 64, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(B // V, nk, heads * 64, generator=g).to(torch.bfloat16).cuda()
    kr, vr = k.repeat_interleave(V, 0).contiguous(), v.repeat_interleave(V, 0).contiguous()
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for scale in (0.125, 0.0):
            plain = ops.attention(q, kr, vr, heads, scale=scale)
            assert torch.equal(ops.attention_grouped(q, kr, vr, heads, kv_group=1, scale=scale).view(torch.int16), plain.view(torch.int16))
            assert torch.equal(ops.attention_grouped(q, k, v, heads, kv_group=V, scale=scale).view(torch.int16), plain.view(torch.int16))
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


def test_grouped_attention_rejects_a_group_that_does_not_divide_the_batch(ops):
    from mvd_amd import _lib as L
    q = torch.zeros(4, 33, 64, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(2, 63, 64, dtype=torch.bfloat16, device="cuda")
    out = torch.empty_like(q)
    import ctypes as C
    rc = L.lib().mvd_op_attention_grouped(C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr()),
                                          C.c_void_p(out.data_ptr()), 4, 1, 33, 63, 64, 64, 64, 64, 0.125, 3, L.stream())
    assert rc != 0 and "does not divide" in L.last_error()
