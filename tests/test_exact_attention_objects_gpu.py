"""Bit-exact tests of object-grouped K/V attention (``ops.attention_objects``, MvdAttnArgs::kv_objects: the views of several
objects in one batch).

The routing problem of exact_util.py for O * g elements with V * nq queries each holds the K/V exactly as the engine stores
them -- element o g + j, object-major -- and its queries and wanted rows, permuted from element-major order into the batch's
[half j][object o][view v] (tests/objects_util.py ``object_views``), are the object forward's rows.  The correct output of batch
row b is V[(q % O) g + q // O][pi] with q = b // V, bit for bit: a row answered from another element (the map left out, the
objects and the halves exchanged, an element off by one) returns that element's V rows, whose values are hashed from the
element index and differ (tests/test_objects_cpu.py shows it on the data).  Every wave-count form (1 / 2 / 4 waves, forced, plan
asserted), generic and engine (prescaled) softmax, the three gain regimes of test_exact_attention_gpu.py, contiguous operands
and views of fused buffers."""
import ctypes as C

import pytest
import torch

import exact_util as X
from tests.objects_util import object_views

pytestmark = pytest.mark.gpu

# O, V, g, heads, nq, nk: (O, V, g) in {(2, 3, 1), (2, 3, 2), (3, 2, 2), (2, 4, 2)}, nq in {33, 144}, nk in {63, 65, 129, 1024},
# heads 1 / 2 / 5 -- each value with each wave count and both softmax forms
CASES = [(2, 3, 1, 1, 33, 63), (2, 3, 2, 2, 144, 65), (3, 2, 2, 5, 33, 129), (2, 4, 2, 2, 144, 1024), (2, 3, 1, 5, 144, 129),
         (3, 2, 2, 1, 144, 63), (2, 4, 2, 5, 33, 1024), (2, 3, 2, 2, 33, 65)]
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


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_object_attention_routes_exactly(ops, case, prescaled, nw_log2):
    from mvd_amd import _lib as L
    O, V, g, heads, nq, nk = case
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for gain in GAINS:
            p = X.routing_problem(O * g, heads, V * nq, nk, gain, prescaled)
            q, k, v, want = object_views(p, O, V, g)
            for what, (q_, k_, v_) in (("contiguous", (q.cuda(), k.cuda(), v.cuda())), ("fused views", fused(q, k, v))):
                got = ops.attention_objects(q_, k_, v_, heads, kv_group=V, kv_objects=O, scale=p.scale)
                plan = ops.last_attention_plan()
                assert plan["waves"] == 1 << nw_log2, plan
                X.assert_same_bits(got, want, f"object attention {case} prescaled {prescaled} waves {1 << nw_log2} gain {gain} {what}")
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


@pytest.mark.parametrize("nw_log2", [-1, 0, 1, 2])
def test_one_object_is_grouped_attention(ops, nw_log2):
    """kv_objects = 1 (and 0) is bit-identical to ops.attention_grouped on generic data; with O = 2, g = 2 the object launch
    equals the grouped launch on K/V re-ordered into the batch's [half][object] order"""
    from mvd_amd import _lib as L
    gen = torch.Generator().manual_seed(15)
    O, V, g, heads, nq, nk = 2, 3, 2, 2, 144, 129
    B = g * O * V
    q = torch.randn(B, nq, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    k = torch.randn(O * g, nk, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(O * g, nk, heads * 64, generator=gen).to(torch.bfloat16).cuda()
    order = [o * g + j for j in range(g) for o in range(O)]            # element read by group q = j O + o
    kb, vb = k[order].contiguous(), v[order].contiguous()
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for scale in (0.125, 0.0):
            grouped = ops.attention_grouped(q, k, v, heads, kv_group=V, scale=scale)
            for one in (0, 1):
                assert torch.equal(ops.attention_objects(q, k, v, heads, kv_group=V, kv_objects=one, scale=scale).view(torch.int16),
                                   grouped.view(torch.int16))
            assert torch.equal(ops.attention_objects(q, k, v, heads, kv_group=V, kv_objects=O, scale=scale).view(torch.int16),
                               ops.attention_grouped(q, kb, vb, heads, kv_group=V, scale=scale).view(torch.int16))
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


@pytest.mark.parametrize("batch,kv_group,kv_objects", [(12, 3, 5), (12, 4, 2), (12, 0, 5), (12, 3, -1)])
def test_object_attention_rejects_a_product_that_does_not_divide_the_batch(ops, batch, kv_group, kv_objects):
    from mvd_amd import _lib as L
    q = torch.zeros(batch, 33, 64, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(batch, 63, 64, dtype=torch.bfloat16, device="cuda")     # (as many elements as any accepted map could read)
    out = torch.empty_like(q)
    rc = L.lib().mvd_op_attention_objects(C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr()),
                                          C.c_void_p(out.data_ptr()), batch, 1, 33, 63, 64, 64, 64, 64, 0.125, kv_group, kv_objects, L.stream())
    assert rc != 0 and "does not divide" in L.last_error(), L.last_error()
