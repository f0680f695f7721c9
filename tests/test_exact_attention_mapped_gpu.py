"""Bit-exact tests of K/V attention by table (``ops.attention_mapped``, MvdAttnArgs::kv_index: ragged view counts per object in
one batch).

The routing problem of exact_util.py for O * g elements with max(V_o) * nq queries each holds the K/V exactly as the engine
stores them -- element o g + j, object-major -- and the queries of batch row (j, o, v) with their wanted rows, laid out in the
ragged [half j][object o][view v] order (tests/ragged_util.py ``ragged_views``), are the ragged forward's rows.  The correct output
of batch row b is V[table[b]][pi], bit for bit: a row answered from another element returns that element's V rows, whose values
are hashed from the element index and differ (tests/test_ragged_cpu.py shows it on the data).  Every wave-count form (1 / 2 / 4
waves, forced, plan asserted), generic and engine (prescaled) softmax, the three gain regimes of test_exact_attention_gpu.py,
contiguous operands and views of fused buffers."""
import ctypes as C

import pytest
import torch

import exact_util as X
from tests.ragged_util import adapter_table, ragged_views

pytestmark = pytest.mark.gpu

# counts, g, heads, nq, nk: counts in {(3, 1), (1, 3), (3, 2, 1), (1, 1, 4)}, g in {1, 2}, nq in {33, 144}, nk in {63, 65, 129, 1024},
# heads 1 / 2 / 5 -- each value with each wave count and both softmax forms
CASES = [((3, 1), 1, 1, 33, 63), ((1, 3), 2, 2, 144, 65), ((3, 2, 1), 2, 5, 33, 129), ((1, 1, 4), 2, 2, 144, 1024), ((3, 2, 1), 1, 5, 144, 129),
         ((1, 3), 1, 1, 144, 63), ((1, 1, 4), 1, 5, 33, 1024), ((3, 1), 2, 2, 33, 65)]
GAINS = (X.LAZY, X.STRICT_LAZY, X.RERUN)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def fused(q, k, v, junk=3.0):
    """q and k / v as column ranges of wider rows (row stride 3 C, as in fused projection outputs), junk in between"""
    B, nq, C_ = q.shape
    E, nk, _ = k.shape
    qb = torch.full((B, nq, 3 * C_), junk, dtype=torch.bfloat16, device="cuda")
    kb = torch.full((E, nk, 3 * C_), junk, dtype=torch.bfloat16, device="cuda")
    qb[:, :, :C_] = q.cuda()
    kb[:, :, C_:2 * C_] = k.cuda()
    kb[:, :, 2 * C_:] = v.cuda()
    return qb[:, :, :C_], kb[:, :, C_:2 * C_], kb[:, :, 2 * C_:]


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_mapped_attention_routes_exactly(ops, case, prescaled, nw_log2):
    from mvd_amd import _lib as L
    counts, g, heads, nq, nk = case
    table = adapter_table(counts, g)
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for gain in GAINS:
            p = X.routing_problem(len(counts) * g, heads, max(counts) * nq, nk, gain, prescaled)
            q, k, v, want = ragged_views(p, counts, g, nq)
            for what, (q_, k_, v_) in (("contiguous", (q.cuda(), k.cuda(), v.cuda())), ("fused views", fused(q, k, v))):
                got = ops.attention_mapped(q_, k_, v_, heads, table, scale=p.scale)
                plan = ops.last_attention_plan()
                assert plan["waves"] == 1 << nw_log2, plan
                X.assert_same_bits(got, want, f"mapped attention {case} prescaled {prescaled} waves {1 << nw_log2} gain {gain} {what}")
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


@pytest.mark.parametrize("nw_log2", [-1, 0, 1, 2])
def test_tables_of_the_arithmetic_maps_are_those_entries_bit_for_bit(ops, nw_log2):
    """on generic data: the table of kv_objects' map is ops.attention_objects, the table b // V ops.attention_grouped, the identity
    table ops.attention -- only the base pointers of a workgroup differ between the forms"""
    from mvd_amd import _lib as L
    from tests.objects_util import element_of
    gen = torch.Generator().manual_seed(16)
    O, V, g, heads, nq, nk = 2, 3, 2, 2, 144, 129
    B = g * O * V
    q = torch.randn(B, nq, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    k = torch.randn(O * g, nk, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(O * g, nk, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    kb = torch.randn(B, nk, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    vb = torch.randn(B, nk, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for scale in (0.125, 0.0):
            objects = ops.attention_objects(q, k, v, heads, kv_group=V, kv_objects=O, scale=scale)
            assert torch.equal(_bits(ops.attention_mapped(q, k, v, heads, [element_of(b // V, O, g) for b in range(B)], scale=scale)), _bits(objects))
            grouped = ops.attention_grouped(q, k, v, heads, kv_group=V, scale=scale)
            assert torch.equal(_bits(ops.attention_mapped(q, k, v, heads, torch.tensor([b // V for b in range(B)]), scale=scale)), _bits(grouped))
            plain = ops.attention(q, kb, vb, heads, scale=scale)
            assert torch.equal(_bits(ops.attention_mapped(q, kb, vb, heads, list(range(B)), scale=scale)), _bits(plain))
            assert not torch.equal(_bits(objects), _bits(grouped))
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
def test_non_monotone_and_constant_tables(ops, prescaled, nw_log2):
    """the elements reversed (a table that no arithmetic on b gives), and every row naming the LAST element (a table read once per
    launch, or per problem instead of per row, returns another element's bits for all rows but a few)"""
    from mvd_amd import _lib as L
    E, heads, nq, nk = 5, 2, 33, 129
    p = X.routing_problem(E, heads, nq, nk, X.LAZY, prescaled)
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        rev = list(range(E - 1, -1, -1))
        got = ops.attention_mapped(p.q[rev].contiguous().cuda(), p.k.cuda(), p.v.cuda(), heads, rev, scale=p.scale)
        X.assert_same_bits(got, p.want[rev].contiguous(), f"reversed table prescaled {prescaled} waves {1 << nw_log2}")
        last = [E - 1] * 7
        q7 = p.q[E - 1:].expand(7, -1, -1).contiguous()
        got = ops.attention_mapped(q7.cuda(), p.k.cuda(), p.v.cuda(), heads, last, scale=p.scale)
        X.assert_same_bits(got, p.want[E - 1:].expand(7, -1, -1).contiguous(), f"constant table prescaled {prescaled} waves {1 << nw_log2}")
        # the same queries against element 0 want other bits: the check above can see a table that is not read
        assert not torch.equal(p.v[0], p.v[E - 1])
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


def _call_mapped(q, kv, out, table, elements, kv_group=None, kv_objects=0):
    from mvd_amd import _lib as L
    B = q.shape[0]
    ptr = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    tab = (C.c_int * B)(*table)
    if kv_group is None:
        return L.lib().mvd_op_attention_mapped(ptr(q), ptr(kv), ptr(kv), ptr(out), B, 1, 33, 63, 64, 64, 64, 64, 0.125, tab, elements, L.stream())
    return L.lib().mvd_debug_attention_mapped_grouped(ptr(q), ptr(kv), ptr(kv), ptr(out), B, 1, 33, 63, 64, 64, 64, 64, 0.125, kv_group,
                                                     kv_objects, tab, elements, L.stream())


@pytest.mark.parametrize("table,kv_group,kv_objects,msg", [
    ([0, 1, 2, 3, 4, 4], None, 0, "entry 4 is 4, outside the 4 K/V elements"),          # an entry equal to kv_elements
    ([0, 1, -1, 3, 0, 0], None, 0, "entry 2 is -1, outside the 4 K/V elements"),         # a negative entry
    ([0, 1, 2, 3, 0, 0], 2, 0, "K/V table together with K/V group 2"),                   # a table together with a group
    ([0, 1, 2, 3, 0, 0], 0, 3, "K/V table together with K/V group 0 / objects 3"),       # ... with an object count
])
def test_mapped_attention_rejections_launch_nothing(ops, table, kv_group, kv_objects, msg):
    """each is refused on the host before anything is uploaded or launched: the output keeps its fill, the launch plan of the
    thread is the one of the launch before"""
    from mvd_amd import _lib as L
    q = torch.zeros(6, 33, 64, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(6, 63, 64, dtype=torch.bfloat16, device="cuda")      # (more elements than any entry that is in range names)
    ok = torch.empty_like(q)
    assert _call_mapped(q, kv, ok, [0, 1, 2, 3, 0, 0], 4) == 0, L.last_error()
    before = ops.last_attention_plan()
    out = torch.full_like(q, 7.0)
    L.lib().mvd_debug_set_attention_nw(2)             # an accepted launch would now record another plan
    try:
        rc = _call_mapped(q, kv, out, table, 4, kv_group, kv_objects)
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)
    assert rc != 0 and msg in L.last_error(), L.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and ops.last_attention_plan() == before
