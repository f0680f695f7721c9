"""test_exact_strides_gpu.py's operands keep what its comparisons rest on -- all on the CPU.

The faults that file exists for are applied to the fp64 reference: a row vector read with the stride of a dense one, or from
column 0 of its buffer, and a weight row read over its padded length.  Each must change what the bitwise comparison sees."""
import ctypes as C

import pytest
import torch

import exact_util as X
import test_exact_conv_gpu as TC
import test_exact_gemm_gpu as TG
import test_exact_strides_gpu as TS


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_embed_and_guard_check_round_trip(dtype):
    g = torch.Generator().manual_seed(3)
    t = torch.randint(-300, 300, (7, 24), generator=g).to(dtype)
    for fill in (X.sentinel(dtype), float("nan"), 3.0):
        buf = X.embed(t, 40, 8, fill)
        assert buf.shape == (7, 40) and buf.dtype == dtype and torch.equal(X._bits(buf[:, 8:32]), X._bits(t))
        guard = torch.cat([buf[:, :8], buf[:, 32:]], 1)
        if torch.is_tensor(fill):
            assert bool((X._bits(guard) == X.SENTINEL_BITS[dtype]).all())
        else:
            assert bool(torch.isnan(guard).all()) if fill != fill else bool((guard == fill).all())
        before = buf.clone()
        buf[:, 8:32] = 0                                     # writing the slice is what a launch does
        assert X.outside_unchanged(buf, before, 8, 24) and not X.outside_unchanged(buf, before, 0, 0)
        for col in (0, 7, 32, 39):                           # one guard element on either side of the slice, at either end
            bad = buf.clone()
            bad[3, col] = 1.0
            assert not X.outside_unchanged(bad, before, 8, 24), col
    # NaN guards compare by bit pattern: a NaN with another payload is a change
    buf = X.embed(t, 40, 8, float("nan"))
    bad = buf.clone()
    bad.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)[0, 0] ^= 1
    assert bool(torch.isnan(bad[0, 0])) and not X.outside_unchanged(bad, buf, 8, 24)


def test_shapes_are_the_sibling_files_shapes():
    """every problem is one whose value ranges and share of bf16 ties test_exact_inputs_cpu.py checks already"""
    assert set(TS.gemm_shapes()) <= set(TG.gemm_shapes())
    assert set(TS.conv_shapes()) <= set(TC.conv_shapes())
    assert TS.GEGLU == TG.GEGLU and TS.CFGS == TG.CFGS and TS.GEGLU_CFGS == TG.GEGLU_CFGS


def _f3_cases():
    out = [(m, n, k, g, m // g) for (m, n, k, g) in TS.gemm_shapes() if g]
    return sorted(set(out))


@pytest.mark.parametrize("m,n,k,groups,rpb", _f3_cases())
def test_f3_wrong_stride_or_offset_changes_the_result(m, n, k, groups, rpb):
    """The row vector is columns [n, 2n) of a [groups][3n] buffer.  Read from column 0 it differs in at least half the elements of
    every group, group 0 included.  Read with the dense stride n (and the right base) group 0 is the same by construction -- row 0
    starts at the base under any stride -- and every other group differs in at least half its elements: every problem with a row
    vector has at least two groups, and a batch-1 launch cannot see this fault at all."""
    assert groups >= 2
    p, acc = X.gemm_problem(m, n, k, groups), X.gemm_acc(m, n, k, groups)
    buf = TS.rowvec_buffer(p.rowvec)
    assert buf.shape == (groups, 3 * n) and torch.equal(buf[:, n:2 * n], p.rowvec)
    assert bool((buf[:, :n] != p.rowvec).all()) and bool((buf[:, 2 * n:] != p.rowvec).all())
    assert buf.min() >= -8 and buf.max() <= 8 and torch.equal(buf, buf.round())
    flat = buf.reshape(-1)
    dense_stride = torch.stack([flat[n + r * n:2 * n + r * n] for r in range(groups)])      # ld = n, base right
    offset0 = buf[:, :n]                                                                     # ld right, offset 0
    right = X.round_once(X.epilogue(acc, p.bias, p.rowvec, rpb))
    for what, rv, first in (("ld = n", dense_stride, 1), ("offset 0", offset0, 0)):
        wrong = X.round_once(X.epilogue(acc, p.bias, rv, rpb))                               # (finite: asserted by round_once)
        differs = (X._bits(wrong) != X._bits(right)).reshape(groups, rpb * n).double().mean(1)
        assert bool((differs[first:] >= 0.5).all()), (what, differs)
    assert torch.equal(dense_stride[0], p.rowvec[0])


@pytest.mark.parametrize("shape", TS.conv_shapes())
def test_f3_conv_wrong_stride_or_offset_changes_the_result(shape):
    B, H, W, cin, cout = shape[:5]
    p = X.conv_problem(*shape)
    acc = X.conv_acc(p.x, p.w)
    buf = TS.rowvec_buffer(p.rowvec)
    flat = buf.reshape(-1)
    dense_stride = torch.stack([flat[cout + r * cout:2 * cout + r * cout] for r in range(B)])
    right = X.round_once(X.epilogue(acc, p.bias, p.rowvec, H * W))
    for rv, first in ((dense_stride, 1), (buf[:, :cout], 0)):
        wrong = X.round_once(X.epilogue(acc, p.bias, rv, H * W))
        differs = (X._bits(wrong) != X._bits(right)).reshape(B, -1).double().mean(1)
        assert B >= 2 and bool((differs[first:] >= 0.5).all()), differs


def _packed_like(w64):
    """what test_exact_strides_gpu.packed_weight builds on the device, in fp64"""
    n, k = w64.shape
    buf = torch.full((n + TS.W_PAD_ROWS, 2 * k), float("nan"), dtype=torch.float64)
    buf[:n, :k] = w64
    return buf


def test_f1_padded_weight_poisons_what_reads_it():
    m, n, (k1, k2), rpbs = TS.EPI
    k = k1 + k2
    p, acc = X.gemm_problem(m, n, k, m // rpbs[0]), X.gemm_acc(m, n, k, m // rpbs[0])
    buf = _packed_like(p.w)
    # the reference: rows [0, n), columns [0, k) -- the padding never enters it
    assert torch.equal(p.a @ buf[:n, :k].T, acc) and not bool(torch.isnan(acc).any())
    # a loader that runs over the full padded row (any k index in [k, 2k) multiplies a NaN)
    assert bool(torch.isnan(torch.cat([p.a, p.a], 1) @ buf[:n].T).all())
    # Ktot taken for the row stride: row r starts at flat element r * k, which is inside the padding for every odd r -- and a
    # buffer resource of N * Ktot elements ends in the middle of the rows [0, n)
    as_dense = buf.reshape(-1)[:n * k].reshape(n, k)
    bad = torch.isnan(p.a @ as_dense.T)
    assert bool(bad[:, 1::2].all()) and not bool(bad[:, 0::2].any())
    # rows beyond n (a row prefix of a taller weight): all padding
    assert bool(torch.isnan(buf[n:]).all()) and buf.shape[0] == n + 64


@pytest.mark.parametrize("c", X.GEGLU_GATES)
def test_f5_padded_weight_poisons_what_reads_it(c):
    from mvd_amd.packing import _geglu_rows
    m, n_out, k = TS.GEGLU
    a, w, bias, val, want = X.geglu_problem(m, n_out, k, c)
    buf = _packed_like(_geglu_rows(w))
    assert torch.equal(buf[:2 * n_out, :k], _geglu_rows(w)) and not bool(torch.isnan(val).any())
    assert bool(torch.isnan(torch.cat([a, a], 1) @ buf[:2 * n_out].T).all())
    assert bool(torch.isfinite(want.float()).all())


def test_sentinel_is_no_reference_value():
    """the guard pattern is finite, so torch keeps its bits in copies, and larger than any value a problem of this file can reach"""
    for dtype in (torch.bfloat16, torch.float32):
        s = X.sentinel(dtype)
        assert bool(torch.isfinite(s)) and int(X._bits(s.reshape(1))[0]) == X.SENTINEL_BITS[dtype]
        assert int(X._bits(s.clone().reshape(1))[0]) == X.SENTINEL_BITS[dtype]
        kmax = max(k for (_, _, k, _) in TS.gemm_shapes())
        assert float(s) > X.partial_sum_bound(kmax) and float(s) > 10 * (3 * TS.GEGLU[2] + 8)
    for (m, n, k, groups) in sorted(set(TS.gemm_shapes())):
        p, acc = X.gemm_problem(m, n, k, groups), X.gemm_acc(m, n, k, groups)
        for out_f32 in (False, True):
            want = X.round_once(X.epilogue(acc, p.bias, p.rowvec, m // groups if groups else 0, p.res), out_f32)
            assert not bool((X._bits(want) == X.SENTINEL_BITS[want.dtype]).any())


def test_refused_pairs_are_well_formed():
    fams = {f.id for f in TS.FAMILIES + TS.GEGLU_FAMILIES}
    for (fam, form), text in TS.REFUSED.items():
        assert fam in fams and form in TS.FORMS and text
    # the engine's own launches -- F1, F2, F3 with the plain layout under the heuristic, on the ping-pong kernel and on the
    # small-M kernels -- are never refused
    assert TS.ENGINE_FORMS and not set(TS.ENGINE_FORMS) & set(TS.REFUSED)
    assert {("cfg-1", "F1"), ("cfg7", "F2"), ("sm0", "F3"), ("sm0_nowait", "F1"), ("sm3_split5", "F2")} <= set(TS.ENGINE_FORMS)
    # slices: EVEN in multiples of 8 elements, ODD in multiples of 4 that are no multiples of 8, and ldres != ldo in both
    assert all(v % 8 == 0 for v in TS.EVEN) and all(v % 4 == 0 for v in TS.ODD) and TS.ODD[0] % 8 and TS.ODD[2] % 8
    assert TS.EVEN[0] != TS.EVEN[2] and TS.ODD[0] != TS.ODD[2]


def test_ping_pong_kernel_leaves_8_byte_strides_to_the_lock_step_tile():
    """gemm_pp.hip stores and fetches 16 bytes per lane at row * ld + a column that is a multiple of 8: mvd_gemm_pp_applicable takes
    row strides that are multiples of 8 elements only (host arithmetic, no GPU)."""
    from mvd_amd import _lib as L
    m, n, (k1, k2), _ = TS.EPI
    k = k1 + k2
    takes = lambda ldw, ldres, ldo: L.lib().mvd_debug_gemm_pp_takes(m, n, k, ldw, ldres, ldo)      # noqa: E731
    assert takes(k, n, n) == 1 and takes(2 * k, n, n) == 1 and takes(k, 0, n) == 1
    assert takes(k, n + TS.EVEN[2], n + TS.EVEN[0]) == 1
    assert takes(k, n + TS.ODD[2], n + TS.ODD[0]) == 0
    assert takes(k, n, n + 4) == 0 and takes(k, n + 4, n) == 0 and takes(k, 0, n + 4) == 0
    assert takes(k, n, n - 8) == -1 and "bad shape" in L.last_error()
