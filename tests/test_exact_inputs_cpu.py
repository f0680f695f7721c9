"""The exact tests' inputs keep their guarantees, and the faults they exist for are visible to them -- all on the CPU.

First half: for every shape the GPU files use (their own case lists are imported), the integer problems stay inside their
value ranges and below 2^24, carry at least 1 % exact bf16 ties where K allows any (K >= 320), and the routing problems leave
at most 2^-12 of softmax mass off the chosen key, reach the keys they must, and have the first-tile lift their regime asks for.

Second half: faults a kernel could have -- one k index dropped, one operand element wrong, one border tap shifted, two V rows
swapped inside a tile, key nk - 1 dropped, truncation instead of round-to-nearest-even -- are applied to a CPU emulation.  Each
one changes the bit pattern the exact tests compare, while the max-norm ``close`` of test_ops_gpu.py, on that file's own
Gaussian inputs, still passes for a wrong operand element of lower-quartile size and for a V swap that one query sees (the
figures for the larger faults, which it does see, are in the tests' docstrings): that is why the exact tests exist."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_util as X
import test_exact_attention_gpu as TA
import test_exact_conv_gpu as TC
import test_exact_gemm_gpu as TG
from test_ops_gpu import close, rnd

TIE_MIN_K = 320            # below, 3 K + 16 hardly reaches the binades where integers are ties (exact_util.py)


def _in_range(t, lo, hi):
    return bool((t == t.round()).all() and t.min() >= lo and t.max() <= hi)


# ------------------------------------------------------------------------------------------------ integer problems
@pytest.mark.parametrize("m,n,k,groups", sorted(set(TG.gemm_shapes())))
def test_gemm_problems_keep_their_guarantees(m, n, k, groups):
    p = X.gemm_problem(m, n, k, groups)
    assert _in_range(p.a, -3, 3) and _in_range(p.w, -1, 1) and _in_range(p.bias, -8, 8) and _in_range(p.res, -16, 16)
    assert p.rowvec is None or _in_range(p.rowvec, -8, 8)
    assert X.partial_sum_bound(k) < 2 ** 24 / 2            # half-integers (alpha = 0.5) below 2^23 are fp32 values too
    acc = X.gemm_acc(m, n, k, groups)
    rpb = m // groups if groups else 0
    for alpha in X.ALPHAS:
        for y in (X.epilogue(acc, p.bias, alpha=alpha), X.epilogue(acc, p.bias, p.rowvec, rpb, p.res, alpha)):
            assert y.abs().max() <= X.partial_sum_bound(k, alpha)
            assert torch.equal(y * 2, (y * 2).round())
            X.round_once(y)                                # asserts that fp64 -> fp32 is exact
            if k >= TIE_MIN_K:
                assert X.tie_share(y) >= 0.01, (alpha, X.tie_share(y))


@pytest.mark.parametrize("shape", sorted(set(TC.conv_shapes())))
def test_conv_problems_keep_their_guarantees(shape):
    B, H, W, cin, cout, sc0, sc1 = shape
    p = X.conv_problem(*shape)
    assert _in_range(p.x, -3, 3) and _in_range(p.w, -1, 1) and _in_range(p.bias, -8, 8) and _in_range(p.rowvec, -8, 8)
    acc = X.conv_acc(p.x, p.w)
    if sc0:
        src = p.s0 if p.s1 is None else torch.cat([p.s0, p.s1], -1)
        assert _in_range(src, -3, 3) and _in_range(p.wsc, -1, 1)
        acc = acc + src @ p.wsc.T
    y = X.epilogue(acc, p.bias)
    assert y.abs().max() <= X.partial_sum_bound(9 * cin + sc0 + sc1, 1.0) < 2 ** 23
    assert X.tie_share(y) >= 0.01, X.tie_share(y)
    up = X.epilogue(X.conv_acc(p.x, p.w, upsample=True), p.bias)
    assert X.tie_share(up) >= 0.01, X.tie_share(up)


def test_up4_weights_of_ternary_taps_are_bf16_values():
    from mvd_amd.packing import pack_up4, up4_weights
    p = X.conv_problem(*TC.UP4_SHAPES[0])
    w4 = up4_weights(p.w)
    assert _in_range(w4, -4, 4)
    co, ci = p.w.shape[:2]
    want = w4.reshape(4, co, ci // 64, 64, 2, 2).permute(0, 1, 2, 4, 5, 3).reshape(4, co, 4 * ci)
    assert torch.equal(pack_up4(X.f32(p.w)).double(), want)


@pytest.mark.parametrize("c", X.GEGLU_GATES)
def test_geglu_gate_constants_stay_within_the_share(c):
    """The kernel's product val * gelu_f32(c), rounded fp32 then bf16, against ONE rounding of val * gelu_fp64(c): the constants
    are chosen so that (on the CPU evaluation of the common.h formula) at most 1 % of the outputs differ, none by more than an ulp."""
    g32 = X.gelu_f32_formula(c)
    assert abs(g32 - X.gelu64(c)) <= 1.5e-7
    m, n_out, k = TG.GEGLU
    _, _, _, val, want = X.geglu_problem(m, n_out, k, c)
    emu = (X.f32(val) * torch.tensor(g32, dtype=torch.float32)).to(torch.bfloat16)
    one_ulp, few, text = X.geglu_ok(emu, want)
    assert one_ulp and few, text
    # the check is sharp enough for what it is for: value and gate rows of one 16-row block exchanged
    wrong = X.round_f64_to_bf16(val.roll(16, 1) * X.gelu64(c))
    assert not all(X.geglu_ok(wrong, want)[:2])


# ------------------------------------------------------------------------------------------------ routing problems
def _routing_cases():
    out = []
    for case in TA.CASES + [TA.LONG]:
        for prescaled in (False, True):
            for gain in TA.GAINS:
                out.append(case + (gain, prescaled, 1, False))
    for (B, heads, nq, nk, nsplit) in TA.SPLIT_CASES:
        for gain in TA.GAINS:
            out.append((B, heads, nq, nk, gain, True, nsplit, False))
    for n in TA.CAUSAL_N:
        for heads in TA.CAUSAL_HEADS:
            for prescaled in (False, True):
                for gain in (X.LAZY, X.RERUN):
                    out.append((2, heads, n, n, gain, prescaled, 1, True))
    return out


@pytest.mark.parametrize("B,heads,nq,nk,gain,prescaled,nsplit,causal", _routing_cases())
def test_routing_problems_keep_their_guarantees(B, heads, nq, nk, gain, prescaled, nsplit, causal):
    p = X.routing_problem(B, heads, nq, nk, gain, prescaled, nsplit, causal)       # (asserts the off-target mass itself)
    assert p.mass <= -12.0
    v = p.v.double()
    assert bool((v.abs() >= 1).all() and (v.abs() < 2).all())
    if causal:
        i = torch.arange(nq)
        assert bool((p.pi <= i).all()) and bool((p.pi == i).any()) and bool((p.pi[..., 1:] == 0).any() or nq == 1)
        return
    # regimes (the first-tile lift only exists beyond the first 64 keys of a range)
    lift = float(p.lift.max())
    if gain == X.LAZY:
        assert lift <= 90.0, lift
    if gain == X.STRICT_LAZY:
        assert lift < 60.0, lift
    if gain == X.RERUN and nk // nsplit >= 129 and B * heads * nq >= 64:
        assert lift >= 140.0, lift
    # reach: per (batch, head) every key where nq >= nk; over all of them the must-hit keys where the queries suffice
    must = X.must_hit(nk, nsplit)
    if nq >= nk:
        for b in range(B):
            for h in range(heads):
                assert len(set(p.pi[b, h].tolist())) == nk
    if B * heads * nq >= len(must):
        assert set(must) <= set(p.pi.flatten().tolist())
    if nq >= 8 and nk >= 8:
        if heads > 1:
            assert not torch.equal(p.pi[:, 0], p.pi[:, 1])
        if B > 1:
            assert not torch.equal(p.pi[0], p.pi[1])


@pytest.mark.parametrize("case", [(2, 2, 33, 63), (1, 2, 200, 333)])
def test_routing_reference_is_the_chosen_row(case):
    """fp64 softmax attention on the routing inputs, rounded once, IS v[pi(i)] -- in both forms"""
    from mvd_amd.packing import QSCALE  # noqa: F401
    for prescaled in (False, True):
        p = X.routing_problem(*case, X.LAZY, prescaled)
        unit = 1.0 if prescaled else 0.125 * X.LOG2E
        ref = X.attention_reference(p.q, p.k, p.v, case[1], unit)
        assert torch.equal(X.round_f64_to_bf16(ref), p.want)


# ------------------------------------------------------------------------------------------------ the faults
def _bits_differ(a, b):
    return not X.same_bits(a, b)[0]


def test_fault_one_k_index_or_one_element():
    """Measured on test_linear_configs' inputs at 77 x 640 x 1024 (bound 2^-7 max|ref| = 0.050): the row's median |a| read as zero
    moves the worst of the row's 640 outputs by 0.067 -- seen -- its lower-quartile |a| by half that -- not seen.  The tolerance
    test catches such a fault for about half of the elements; the exact test for every non-zero one."""
    m, n, k = 77, 640, 1024
    p = X.gemm_problem(m, n, k)
    want = X.round_once(X.epilogue(X.gemm_acc(m, n, k), p.bias))
    k0, r0 = 517, 40
    # a kernel that skips k index k0 (all rows), and one that reads ONE element of A wrong (here: as zero)
    a_k = p.a.clone(); a_k[:, k0] = 0                                        # noqa: E702
    k1 = int(p.a[r0].abs().argmax())
    a_e = p.a.clone(); a_e[r0, k1] = 0                                       # noqa: E702
    for a_bad in (a_k, a_e):
        assert _bits_differ(X.round_once(X.epilogue(a_bad @ p.w.T, p.bias)), want)
    a, w, bias = rnd(m, k, seed=1), rnd(n, k, scale=1 / math.sqrt(k), seed=2), rnd(n, seed=3, dtype=torch.float32)
    ref = a.float() @ w.float().T + bias
    bad = a.clone()
    bad[r0, a[r0].float().abs().argsort()[k // 4]] = 0                       # the lower quartile of the row's |a|
    got = (bad.float() @ w.float().T + bias).to(torch.bfloat16)
    assert _bits_differ(got, ref.to(torch.bfloat16))
    close(got, ref, what="one wrong k element, Gaussian inputs")


def test_fault_one_border_tap_shifted():
    """(On test_conv3x3's Gaussian inputs at this shape the same fault with a median-sized pixel moves the worst output by 0.10
    against a bound of 0.051: the tolerance test sees the larger half of such faults, the exact test every non-zero one.)"""
    shape = (2, 16, 16, 64, 128)
    p = X.conv_problem(*shape)
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w), p.bias))
    # the tap above pixel (0, 3) of image 0 reads pixel (0, 3) itself instead of the zero padding, in one channel
    ch = int(p.x[0, 0, 3].abs().argmax())
    xp = F.pad(p.x.permute(0, 3, 1, 2), (1, 1, 1, 1)).clone()
    xp[0, ch, 0, 4] = xp[0, ch, 1, 4]
    assert _bits_differ(X.round_once(X.epilogue(F.conv2d(xp, p.w).permute(0, 2, 3, 1), p.bias)), want)


def test_fault_v_rows_swapped_or_last_key_dropped():
    """Two V rows of one tile exchanged, and key nk - 1 left out.  On test_attention's Gaussian inputs at 1 x 5 x 1024 x 1024
    (bound 2^-6 max|ref| = 0.0053) a swap that EVERY query sees is found by the tolerance test too (0.087: some query always
    weighs one of the two keys at thirty times 1 / nk); a swap that one query sees -- one lane's P / V pairing -- is not, for a
    query that weighs the two keys as the median query does.  The exact test fails in both cases."""
    B, heads, nq, nk = 1, 5, 1024, 1024                                       # test_attention's multi-tile case
    j1, j2 = 70, 77                                                           # two rows of the second 64-key tile
    p = X.routing_problem(B, heads, nq, nk, X.LAZY, False)
    unit = 0.125 * X.LOG2E
    assert torch.equal(X.round_f64_to_bf16(X.attention_reference(p.q, p.k, p.v, heads, unit)), p.want)
    swapped = X.round_f64_to_bf16(X.attention_reference(p.q, p.k, p.v, heads, unit, swap=(j1, j2)))
    assert _bits_differ(swapped, p.want)
    one = p.want.clone()
    i0 = int((p.pi[0, 0] == j1).nonzero()[0])                                 # the query of head 0 that picks key j1
    one[0, i0, :64] = swapped[0, i0, :64]
    assert _bits_differ(one, p.want)
    assert _bits_differ(X.round_f64_to_bf16(X.attention_reference(p.q, p.k, p.v, heads, unit, drop=nk - 1)), p.want)
    C = heads * 64
    q, k, v = rnd(B, nq, C, seed=1), rnd(B, nk, C, seed=2), rnd(B, nk, C, seed=3)
    ref = X.attention_reference(q, k, v, heads, unit)
    good = X.round_f64_to_bf16(ref)
    swapped = X.round_f64_to_bf16(X.attention_reference(q, k, v, heads, unit, swap=(j1, j2)))
    s = (q.double()[0, :, :64] @ k.double()[0, :, :64].T) * unit              # head 0
    wgt = torch.softmax(s * math.log(2.0), -1)[:, [j1, j2]].sum(-1)
    i0 = int(wgt.argsort()[nq // 2])
    one = good.clone()
    one[0, i0, :64] = swapped[0, i0, :64]
    assert _bits_differ(one, good)
    close(one, ref.float(), tol=2 ** -6, what="two V rows swapped for one query, Gaussian inputs")


def test_fault_truncation_instead_of_nearest_even():
    m, n, k = 300, 640, 320
    p = X.gemm_problem(m, n, k)
    y = X.epilogue(X.gemm_acc(m, n, k), p.bias)
    want = X.round_once(y)
    assert _bits_differ(X.truncate_to_bf16(y), want)
    # round-half-up (or a double rounding through a wider format that ends on a tie) differs on the ties alone
    f = X.f32(y).contiguous().view(torch.int32)
    half_up = ((f + 0x8000) & -65536).view(torch.float32).to(torch.bfloat16)
    assert _bits_differ(half_up, want)
    assert float((half_up.double() - want.double()).abs().max()) > 0 and X.tie_share(y) >= 0.01
    # ... while truncation of test_linear_configs' Gaussian outputs costs less than one ulp of each: inside the tolerance
    a, w, bias = rnd(m, k, seed=1), rnd(n, k, scale=1 / math.sqrt(k), seed=2), rnd(n, seed=3, dtype=torch.float32)
    ref = a.float() @ w.float().T + bias
    close(X.truncate_to_bf16(ref.double()), ref, what="truncated outputs, Gaussian inputs")
