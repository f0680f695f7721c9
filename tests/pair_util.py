"""Cases and data of the two-problem attention launches (MvdAttnArgs::nprob = 2), shared by tests/test_attention_pair_cpu.py -- which
shows on the data that the faults in question change wanted rows -- and tests/test_exact_attention_pair_gpu.py.

A case is (layout, B or None, heads, nq0, nk0, nq1, nk1, nsplit).  Layouts: "plain" (every batch element its own K/V in both
problems) and the four map combinations the engine issues for the shared forwards, problem 0 holding the text K/V and problem 1
the reference K/V as in attn2 (``LAYOUTS``).  The data are exact_util.routing_pair's over the K/V ELEMENTS of each problem, with as
many queries per element as batch rows read it; tests/objects_util.py and tests/ragged_util.py permute them into batch order.

Plain helper module (like exact_util.py), no fixtures; nothing here touches the code under test."""
from types import SimpleNamespace

import exact_util as X
from tests.objects_util import element_of, object_views
from tests.ragged_util import adapter_table, ragged_views, text_table

# ---- (a) unsplit: B, heads, nq0, nk0, nq1, nk1
ROUTE = [(2, 2, 144, 144, 144, 72),      # self with a half-length reference; 8 pairs: the swizzled decode
         (1, 5, 200, 77, 200, 200),      # text with reference; 10 pairs: the plain decode; a ragged last query block
         (3, 1, 33, 63, 33, 129),
         (1, 2, 144, 1024, 144, 65),     # one problem finishes fifteen tiles before the other
         (2, 1, 200, 64, 200, 65),
         (1, 2, 200, 129, 33, 333)]      # different query counts: the grid is sized by the larger
# ---- (b) split-KV: B, heads, nq0, nq1, nk0, nk1, nsplit
SPLIT = [(1, 2, 200, 200, 128, 192, 2),       # 8 (pair, range)s: swizzled
         (2, 2, 144, 144, 192, 1111, 3),      # 24: swizzled
         (1, 5, 200, 200, 1111, 1111, 2),     # 20: plain
         (1, 2, 200, 33, 256, 128, 2)]
# ---- (c) maps that differ between the problems: layout, heads, nq, nk0, nk1
V_, G_, O_, COUNTS = 3, 2, 2, (3, 2, 1)
MAPPED = [("views_self", 2, 33, 65, 129),      # 24 pairs: swizzled
          ("views_cross", 1, 33, 63, 129),     # 12: plain
          ("objects", 2, 33, 129, 65),         # 48: swizzled
          ("ragged", 1, 33, 63, 65)]           # 24: swizzled
MAPPED_SPLIT = ("views_self", 1, 33, 128, 192, 2)     # a group on problem 1 and a split


def route_case(c):
    B, heads, nq0, nk0, nq1, nk1 = c
    return ("plain", B, heads, nq0, nk0, nq1, nk1, 1)


def split_case(c):
    B, heads, nq0, nq1, nk0, nk1, nsplit = c
    return ("plain", B, heads, nq0, nk0, nq1, nk1, nsplit)


def mapped_case(c, nsplit=1):
    layout, heads, nq, nk0, nk1 = c[:5]
    return (layout, None, heads, nq, nk0, nq, nk1, c[5] if len(c) > 5 else nsplit)


def all_cases():
    """every routing case of the GPU file"""
    return [route_case(c) for c in ROUTE] + [split_case(c) for c in SPLIT] + [mapped_case(c) for c in MAPPED] + [mapped_case(MAPPED_SPLIT)]


def _identity(p):
    return p.q, p.k, p.v, p.want


def _text_order(p, O, g):
    """the elements of p renumbered so that ragged_views, which takes the queries of batch row (j, o, v) from element o g + j, takes
    them from element j O + o -- the text rows' order; K/V stay where they are"""
    perm = [j * O + o for o in range(O) for j in range(g)]
    return SimpleNamespace(q=p.q[perm], want=p.want[perm], k=p.k, v=p.v)


def layout(name, B=None):
    """-> (batch, per problem (elements, batch rows per element at the most, map arguments of ops.attention_pair, the element every
    batch row reads, permutation into batch order))"""
    V, g, O = V_, G_, O_
    if name == "plain":
        one = (B, 1, {}, list(range(B)), _identity)
        return B, (one, one)
    if name in ("views_self", "views_cross"):       # batch [half j][view v]; K/V elements: one per half
        B = g * V
        grouped = (g, V, {"kv_group": V}, [b // V for b in range(B)], lambda p: object_views(p, 1, V, g))
        own = (B, 1, {}, list(range(B)), _identity)
        return B, ((own if name == "views_self" else grouped), grouped)
    if name == "objects":                             # batch [half j][object o][view v]; text rows [half][object], reference [object][half]
        B = g * O * V
        text = (g * O, V, {"kv_group": V}, [b // V for b in range(B)], lambda p: object_views(p, 1, V, g * O))
        ref = (O * g, V, {"kv_group": V, "kv_objects": O}, [element_of(b // V, O, g) for b in range(B)], lambda p: object_views(p, O, V, g))
        return B, (text, ref)
    if name == "ragged":
        counts, n = COUNTS, len(COUNTS)
        B = g * sum(counts)
        tt, at = text_table(counts, g), adapter_table(counts, g)
        text = (g * n, max(counts), {"kv_index": tt}, tt, lambda p: ragged_views(_text_order(p, n, g), counts, g, p.q.shape[1] // max(counts)))
        ref = (n * g, max(counts), {"kv_index": at}, at, lambda p: ragged_views(p, counts, g, p.q.shape[1] // max(counts)))
        return B, (text, ref)
    raise ValueError(name)


def build(case, gain, prescaled):
    """the data of one case: ``B``, ``heads``, ``nsplit``, ``scale`` and ``prob`` = two namespaces with ``q`` (B, nq, C) and ``want`` in batch
    order, ``k`` / ``v`` (E, nk, C), ``nq``, ``nk``, ``table`` (the element every batch row reads) and ``map`` (the arguments that say so
    to ops.attention_pair)"""
    name, B, heads, nq0, nk0, nq1, nk1, nsplit = case
    B, lay = layout(name, B)
    (E0, m0, _, _, _), (E1, m1, _, _, _) = lay
    ps = X.routing_pair(E0, E1, heads, m0 * nq0, nk0, m1 * nq1, nk1, gain, prescaled, nsplit)
    prob = []
    for p, (E, m, kw, table, to_batch), nq, nk in zip(ps, lay, (nq0, nq1), (nk0, nk1)):
        q, k, v, want = to_batch(p)
        assert q.shape == (B, nq, heads * 64) and k.shape == (E, nk, heads * 64) and len(table) == B and max(table) == E - 1
        prob.append(SimpleNamespace(q=q, k=k, v=v, want=want, nq=nq, nk=nk, table=table, map=kw, lift=p.lift))
    return SimpleNamespace(B=B, heads=heads, nsplit=nsplit, scale=ps[0].scale, prob=prob)


def pairs(case):
    """(pair, key range)s the kernel's block decode counts for this case: its swizzled branch takes multiples of 8"""
    name, B, heads = case[:3]
    B, _ = layout(name, B)
    return heads * B * 2 * case[7]
