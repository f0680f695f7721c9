"""Bit-exact attention tests: routing problems (exact_util.py) whose correct output is v[pi(i)], bit for bit.  Every query
picks ONE key -- key 0, key nk - 1, both sides of every 64-key tile and split boundary, every key where there are queries
enough -- so a key dropped or doubled at a boundary, two V rows swapped inside a tile, a wrong row of the ragged last tile or a
wrong split-KV merge shows as a wrong row; at nk = 1024 the tolerance tests see none of these (each key weighs 1 / nk).

Three regimes by the query gain: LAZY (the engine form may keep its first tile's maximum: P = 2^lift, lift <= 90),
STRICT_LAZY (lift < 60: below the kernel's acceptance bound of 2^64 on the denominators, so the unchecked loop's own result is
stored) and RERUN (lift >= 140: the unchecked loop overflows and the workgroup takes the checked loop).

Every launch here has ONE problem (every mvd_op_attention* entry sets nprob = 1).  The two-problem launches of the image-conditioned
transformer blocks -- the pair decode of the workgroup id, the per-problem fields, the split-KV workspace over both problems -- are
covered by test_exact_attention_pair_gpu.py through ops.attention_pair."""
import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

# B, heads, nq, nk: every nq of {4, 33, 144, 200}, every nk of {4, 63, 64, 65, 77, 129, 333, 1024}, heads 1 / 2 / 5, batch 1 / 2
CASES = [(1, 1, 4, 4), (2, 2, 33, 63), (1, 5, 144, 64), (2, 1, 200, 65), (1, 2, 33, 77), (2, 5, 144, 129), (1, 2, 200, 333),
         (2, 2, 200, 1024), (1, 1, 4, 1024)]
LONG = (1, 2, 200, 4096)
GAINS = (X.LAZY, X.STRICT_LAZY, X.RERUN)
SPLIT_CASES = [(1, 2, 200, 128, 2), (2, 5, 33, 192, 2), (1, 2, 144, 192, 3), (2, 2, 200, 1111, 2), (1, 5, 200, 1111, 3)]   # ..., nk, nsplit
CAUSAL_N = [1, 13, 64, 65, 77, 96]
CAUSAL_HEADS = [4, 16]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def fused_views(p, junk=3.0):
    """q and k / v as column ranges of wider rows (row stride 3 * heads * 64, as in a fused QKV buffer); one buffer when nq == nk"""
    B, nq, C = p.q.shape
    nk = p.k.shape[1]
    qb = torch.full((B, nq, 3 * C), junk, dtype=torch.bfloat16, device="cuda")
    kb = qb if nq == nk else torch.full((B, nk, 3 * C), junk, dtype=torch.bfloat16, device="cuda")
    qb[:, :, :C] = p.q.cuda()
    kb[:, :, C:2 * C] = p.k.cuda()
    kb[:, :, 2 * C:] = p.v.cuda()
    return qb[:, :, :C], kb[:, :, C:2 * C], kb[:, :, 2 * C:]


def run_case(ops, case, prescaled, nw_log2):
    from mvd_amd import _lib as L
    B, heads, nq, nk = case
    L.lib().mvd_debug_set_attention_nw(nw_log2)
    try:
        for gain in GAINS:
            p = X.routing_problem(B, heads, nq, nk, gain, prescaled)
            for what, (q, k, v) in (("contiguous", (p.q.cuda(), p.k.cuda(), p.v.cuda())), ("fused views", fused_views(p))):
                got = ops.attention(q, k, v, heads, scale=p.scale)
                plan = ops.last_attention_plan()
                assert plan["waves"] == 1 << nw_log2, plan
                X.assert_same_bits(got, p.want, f"attention {case} prescaled {prescaled} waves {1 << nw_log2} gain {gain} {what}")
    finally:
        L.lib().mvd_debug_set_attention_nw(-1)


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_attention_routes_exactly(ops, case, prescaled, nw_log2):
    run_case(ops, case, prescaled, nw_log2)


@pytest.mark.parametrize("nw_log2", [0, 1, 2])
@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_routes_exactly_4096_keys(ops, prescaled, nw_log2):
    run_case(ops, LONG, prescaled, nw_log2)


@pytest.mark.parametrize("case", SPLIT_CASES)
def test_attention_split_routes_exactly(ops, case):
    """split-KV: the chosen keys lie in the first range, in the last, and on both sides of every range boundary (must_hit)"""
    B, heads, nq, nk, nsplit = case
    for gain in GAINS:
        p = X.routing_problem(B, heads, nq, nk, gain, True, nsplit)
        for what, (q, k, v) in (("contiguous", (p.q.cuda(), p.k.cuda(), p.v.cuda())), ("fused views", fused_views(p))):
            got = ops.attention_split(q, k, v, heads, nsplit)
            X.assert_same_bits(got, p.want, f"split-KV attention {case} gain {gain} {what}")


@pytest.mark.parametrize("heads", CAUSAL_HEADS)
@pytest.mark.parametrize("n", CAUSAL_N)
def test_attention_causal_routes_exactly(ops, n, heads):
    """pi(i) <= i, cycling through pi(i) = i (the diagonal of the mask), pi(i) = 0 and a key in between"""
    for prescaled in (False, True):
        for gain in (X.LAZY, X.RERUN):
            p = X.routing_problem(2, heads, n, n, gain, prescaled, 1, True)
            for what, (q, k, v) in (("contiguous", (p.q.cuda(), p.k.cuda(), p.v.cuda())), ("fused views", fused_views(p))):
                got = ops.attention_causal(q, k, v, heads, scale=p.scale)
                X.assert_same_bits(got, p.want, f"causal attention n {n} heads {heads} prescaled {prescaled} gain {gain} {what}")
