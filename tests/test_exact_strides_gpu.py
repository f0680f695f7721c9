"""Bit-exact tests of the call forms the ENGINE issues and mvd_op_linear / ops.conv3x3's dense arguments could not build: a weight
read with a row stride beyond K, outputs and residuals that are column slices of wider buffers, in-place launches (res == out)
and a row vector that is a column slice of the fused time-embedding projection -- through ops.linear_ld (mvd_op_linear_ld) and
ops.conv3x3, on the integer problems and the shapes of test_exact_gemm_gpu.py / test_exact_conv_gpu.py, compared bitwise with the
fp64 reference rounded once.  What a dense launch cannot see fails here: a loader that takes Ktot for the weight's row stride or a
buffer resource sized N * Ktot reads the NaN padding, an epilogue that takes N for the row vector's (or the output's, or the
residual's) stride reads the neighbouring block's integers or writes the guard columns.

Forms.  F1: the packed out-projection with the adapter off -- w is the left half of an [n + 64][2k] buffer, everything else in it
bf16 NaN; bias, in place.  F2: the adapter on -- two sources a | a2, ldw = k1 + k2, in place.  F3: the row vector is columns
[n, 2n) of a [groups][3n] fp32 buffer whose other blocks hold other integers of the same range (``rowvec_buffer``).  F4: out is
a column slice of a buffer filled with a sentinel bit pattern, res a slice of another buffer with another stride; the guard
columns keep their bits.  Strides and offsets are multiples of 8 elements, and (``ODD``) of 4 only: every family but the
ping-pong kernels moves at most 8 bytes per bf16 access (16 per fp32 access, where 4 elements are 16 bytes), and
mvd_gemm_pp_applicable leaves such a launch to the lock-step tile of the same shape (test_exact_strides_cpu.py asks it).
F5: GEGLU with ldw = 2k and ldo > n / 2.  ALL: F1 + F3 + F4 at every alpha, and once in place on a slice.

Families: the tiled kernels by force_cfg (7 = the ping-pong kernel, 6 its GEGLU form), the small-M tiles 0-6 at ring depth 3
with the plain and the blocked weight layout, split-K with the separate reduce pass, with the in-kernel combine and with the
no-wait combine.  No pair of family and form is skipped: the pairs a family refuses stand in REFUSED with the text of the
refusal, ``attempt`` asserts that exactly those raise -- and launch nothing -- and that every other pair runs.  The ReLU forms are
not here: ops.linear_relu is dense by construction and mvd_op_linear_ld does not expose ``relu``."""
from types import SimpleNamespace

import pytest
import torch

import exact_util as X
import test_exact_conv_gpu as TC
import test_exact_gemm_gpu as TG

pytestmark = pytest.mark.gpu

CFGS = [-1, 2, 3, 4, 5, 7, 10, 11, 12, 13]
GEGLU_CFGS = [-1, 3, 4, 5, 6, 11, 12, 13]
SM_TILES = list(range(7))
W_PAD_ROWS = 64
NAN = float("nan")
# (m, n, (k1, k2), rows_per_batch values) of the dense problems: the sibling file's shapes
EPI = (TG.EPI[0], TG.EPI[1], (TG.EPI[2], TG.EPI[3]), TG.EPI_RPB)
SPLITK = (TG.SPLITK[0], TG.SPLITK[1], (TG.SPLITK[2] // 2, TG.SPLITK[2] // 2), (TG.SPLITK[3],))
SM_SPLITK = (TG.SM_SPLITK[0], TG.SM_SPLITK[1], (TG.SM_SPLITK[2] // 2, TG.SM_SPLITK[2] // 2), (TG.SM_SPLITK[3],))
NOWAIT = (TG.NOWAIT[0], TG.NOWAIT[1], (TG.NOWAIT[2] // 2, TG.NOWAIT[2] // 2), (0,))        # (no row vector: the sibling's problem has none)
GEGLU = TG.GEGLU
FUSION, SPLIT_TILED, SPLIT_SM = TC.FUSION[:5] + (TC.FUSION[5], 0), TC.SPLIT_TILED, TC.SPLIT_SM
# slices of F4 / F5 / ALL: (ldo - n, column offset of out, ldres - n, column offset of res)
EVEN = (72, 40, 24, 8)                       # multiples of 8 elements
ODD = (12, 4, 20, 12)                        # multiples of 4 only: the smallest the launcher admits beyond EVEN
SLICES = {"even": EVEN, "odd": ODD}


def gemm_shapes():
    """(m, n, k, rowvec groups) of every integer GEMM problem of this file: a subset of test_exact_gemm_gpu.gemm_shapes()"""
    out = []
    for m, n, (k1, k2), rpbs in (EPI, SPLITK, SM_SPLITK, NOWAIT):
        out += [(m, n, k1 + k2, m // r if r else 0) for r in rpbs]
    return out


def conv_shapes():
    return [FUSION, SPLIT_TILED + (0, 0), SPLIT_SM + (0, 0)]


def sm_cfg(tile, depth=3):
    return 100 + 10 * tile + depth


def _fam(id, shape, blocked=False, **kw):
    return SimpleNamespace(id=id, shape=shape, blocked=blocked, kw=kw)


TILED = [_fam(f"cfg{c}", EPI, force_cfg=c) for c in CFGS]
SM = [_fam(f"sm{t}" + ("_blocked" if b else ""), EPI, blocked=b, force_cfg=sm_cfg(t)) for t in SM_TILES for b in (False, True)]
SPLIT_REDUCE = [_fam(f"split3_cfg{c}", SPLITK, force_cfg=c, splitk=3) for c in [-1, 7, 10, 13]]
SPLIT_SM_FAMS = [_fam(f"sm{t}_split{s}", SM_SPLITK, force_cfg=sm_cfg(t), splitk=s) for t in [0, 3, 6] for s in [2, 5]]
NOWAIT_FAM = [_fam("sm0_nowait", NOWAIT, force_cfg=sm_cfg(0, 4), splitk=TG.NOWAIT[3])]
SPLIT = SPLIT_REDUCE + SPLIT_SM_FAMS + NOWAIT_FAM
FAMILIES = TILED + SM + SPLIT
GEGLU_FAMILIES = [_fam(f"cfg{c}", None, force_cfg=c) for c in GEGLU_CFGS] + [f for f in SM + SPLIT]
FORMS = ("F1", "F2", "F3", "F4", "F5", "ALL")

# (family, form) -> a piece of the message the refusal carries.  Rules:
# * the blocked weight layout stores [N / 32][K / 64] blocks: it has no row stride, so a weight whose rows are 2k apart (F1, F5,
#   ALL) cannot be given in it (gemm_sm.hip mvd_gemm_sm_applicable / mvd_launch_gemm_sm: w_blocked needs ldw == Ktot);
# * GEGLU pairs value / gate tiles inside a wave: the 160-wide small-M tiles 4 and 5 give a wave 5 column tiles, an odd count;
# * GEGLU has no split-K form in any family (mvd_launch_gemm: its epilogue is not linear in the partial sums).
REFUSED = {}
for _f in SM:
    if _f.blocked:
        REFUSED.update({(_f.id, form): "blocked weight layout has no row stride" for form in ("F1", "F5", "ALL")})
REFUSED.update({(f"sm{t}", "F5"): "does not take" for t in (4, 5)})
REFUSED.update({(_f.id, "F5"): "bad split-K request" for _f in SPLIT})
# the engine's own launches: the heuristic, the ping-pong kernel and the small-M kernels with the plain layout
ENGINE_FORMS = [(f.id, form) for f in TILED + SM + SPLIT for form in ("F1", "F2", "F3")
                if not f.blocked and (f.kw["force_cfg"] in (-1, 7) or f.kw["force_cfg"] >= 100)]

ids = lambda fams: [f.id for f in fams]   # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


# ------------------------------------------------------------------------------------------------ operands
def rowvec_buffer(rv64):
    """(groups, n) integers in [-8, 8] -> (groups, 3n): [other | rv | another], every element of the two outer blocks an integer of
    the same range that differs from the one of ``rv`` in its column"""
    other = lambda d: (rv64 + 8 + d) % 17 - 8     # noqa: E731
    return torch.cat([other(5), rv64, other(11)], 1)


def packed_weight(w):
    """device (n, k) bf16 -> the view [:n, :k] of an [n + W_PAD_ROWS][2k] buffer that is NaN everywhere else"""
    n, k = w.shape
    buf = torch.full((n + W_PAD_ROWS, 2 * k), NAN, dtype=w.dtype, device=w.device)
    buf[:n, :k] = w
    return buf[:n, :k]


def problem(fam, rpb):
    m, n, (k1, k2), _ = fam.shape
    groups = m // rpb if rpb else 0
    return X.gemm_problem(m, n, k1 + k2, groups), X.gemm_acc(m, n, k1 + k2, groups)


def launch(ops, fam, a, w, packed, **kw):
    """ops.linear_ld of family ``fam`` with the dense device weight ``w`` given in the form's layout: ``packed`` = rows 2k apart"""
    if fam.blocked:
        from mvd_amd.packing import block_weight
        n, k = w.shape
        return ops.linear_ld(a, block_weight(w), blocked=(n, k, 2 * k if packed else k), **fam.kw, **kw)
    return ops.linear_ld(a, packed_weight(w) if packed else w, **fam.kw, **kw)


def attempt(ops, fam, form, fn, buf=None):
    """fn() launches one (family, form) pair.  A pair listed in REFUSED must raise with its message and leave ``buf`` as it was
    (nothing launched); every other pair must run.  Returns fn()'s result, or None for a refusal."""
    from mvd_amd._lib import MvdError
    if (fam.id, form) not in REFUSED:
        return fn()
    before = None if buf is None else buf.clone()
    with pytest.raises(MvdError) as e:
        fn()
    assert REFUSED[(fam.id, form)] in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert buf is None or X.outside_unchanged(buf, before, 0, 0), f"{fam.id} {form}: refused, but the output was written"
    return None


_HEURISTIC = {}


def heuristic_cfg(ops, m, n, k, geglu, splitk):
    """tile config the heuristic gives the DENSE launch of this shape (mvd_op_linear, as test_exact_gemm_gpu.py runs it)"""
    key = (m, n, k, geglu, splitk)
    if key not in _HEURISTIC:
        z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")     # noqa: E731
        ops.linear(z(m, k), z(n, k), geglu=geglu, splitk=splitk)
        _HEURISTIC[key] = ops.last_gemm_plan()["cfg"]
    return _HEURISTIC[key]


def check_route(ops, fam, gemm=None):
    """the launch that just ran took the family's kernel; under the heuristic, the tile the dense launch of the same (m, n, k) takes"""
    plan = ops.last_gemm_plan()
    cfg, splitk = fam.kw["force_cfg"], fam.kw.get("splitk", 1)
    if cfg < 0:
        m, n, k, geglu = gemm if gemm else (fam.shape[0], fam.shape[1], sum(fam.shape[2]), False)
        want = heuristic_cfg(ops, m, n, k, geglu, splitk)
    else:
        want = cfg if cfg >= 100 or cfg < 8 else cfg - 8
    ok = plan["cfg"] == want and plan["splitk"] == splitk
    if fam.id == "sm0_nowait":
        m, n = fam.shape[:2]
        ok = ok and plan["grid"] == (m // 64) * (n // 64) * splitk and plan["nowait"] == 1
    assert ok, (fam.id, plan)
    return plan


def sliced(t, pad, off, fill):
    """(buffer, view) with the device tensor ``t`` in columns [off, off + n) of a buffer ``pad`` wider"""
    buf = X.embed(t, t.shape[1] + pad, off, fill)
    return buf, buf[:, off:off + t.shape[1]]


# ------------------------------------------------------------------------------------------------ F1, F2: in place
@pytest.mark.parametrize("fam", FAMILIES, ids=ids(FAMILIES))
def test_f1_packed_weight_in_place(ops, fam):
    m, n, (k1, k2), rpbs = fam.shape
    p, acc = problem(fam, rpbs[0])
    want = X.round_once(X.epilogue(acc, p.bias, res=p.res))
    a, w, bias, h = X.dev(p.a), X.dev(p.w), X.dev32(p.bias), X.dev(p.res)
    got = attempt(ops, fam, "F1", lambda: launch(ops, fam, a, w, True, bias=bias, res=h, out=h), h)
    if got is None:
        return
    check_route(ops, fam)
    X.assert_same_bits(h, want, f"{fam.id} F1: ldw = 2k with NaN padding, in place")


@pytest.mark.parametrize("fam", FAMILIES, ids=ids(FAMILIES))
def test_f2_two_sources_in_place(ops, fam):
    m, n, (k1, k2), rpbs = fam.shape
    p, acc = problem(fam, rpbs[0])
    want = X.round_once(X.epilogue(acc, p.bias, res=p.res))
    a, a2, w, bias, h = X.dev(p.a[:, :k1]), X.dev(p.a[:, k1:]), X.dev(p.w), X.dev32(p.bias), X.dev(p.res)
    attempt(ops, fam, "F2", lambda: launch(ops, fam, a, w, False, a2=a2, bias=bias, res=h, out=h), h)
    check_route(ops, fam)
    X.assert_same_bits(h, want, f"{fam.id} F2: a | a2, in place")


# ------------------------------------------------------------------------------------------------ F3: the row vector is a column slice
@pytest.mark.parametrize("fam", TILED + SM, ids=ids(TILED + SM))
def test_f3_row_vector_slice(ops, fam):
    m, n, (k1, k2), rpbs = fam.shape
    for rpb in rpbs:
        p, acc = problem(fam, rpb)
        want = X.round_once(X.epilogue(acc, p.bias, p.rowvec, rpb))
        rv = X.dev32(rowvec_buffer(p.rowvec))[:, n:2 * n]
        got = attempt(ops, fam, "F3", lambda: launch(ops, fam, X.dev(p.a), X.dev(p.w), False, bias=X.dev32(p.bias), rowvec=rv, rows_per_batch=rpb))
        check_route(ops, fam)
        X.assert_same_bits(got, want, f"{fam.id} F3: row vector = columns [n, 2n) of [groups][3n], rows_per_batch {rpb}")


def conv_f3(ops, cfg, shape, splitk, with_res):
    B, H, W, cin, cout = shape[:5]
    p = X.conv_problem(*shape)
    res64 = p.x * 5.0 + 1.0 if with_res else None          # (cin == cout: integers in [-14, 16], as test_exact_conv_gpu.py)
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w), p.bias, p.rowvec, H * W, res64))
    x, bias, res = X.dev(p.x), X.dev32(p.bias), X.dev(res64)
    rv = X.dev32(rowvec_buffer(p.rowvec))[:, cout:2 * cout]
    got = TC.layouts(ops, cfg, TC.pack(p.w), lambda w, blk: ops.conv3x3(x, w, bias, rowvec=rv, res=res, force_cfg=cfg, splitk=splitk, blocked=blk))
    plan = ops.last_gemm_plan()
    if cfg < 0:                                             # the heuristic: the tile of the dense-row-vector launch (test_exact_conv_gpu.py)
        ops.conv3x3(x, X.dev(TC.pack(p.w)), bias, rowvec=X.dev32(p.rowvec), res=res, splitk=splitk)
        route = ops.last_gemm_plan()["cfg"]
    else:
        route = cfg if cfg >= 100 or cfg < 8 else cfg - 8
    ok = plan["splitk"] == splitk and plan["cfg"] == route
    assert ok, (plan, route)
    X.assert_same_bits(got, want, f"conv3x3 cfg {cfg} split-K {splitk}: row vector = columns [cout, 2 cout) of [B][3 cout]")


@pytest.mark.parametrize("cfg", TC.FUSION_CFGS + [sm_cfg(t, 4) for t in TC.SM_TILES if FUSION[4] % TC.SM_BN[t] == 0])
def test_f3_conv_row_vector_slice_with_residual(ops, cfg):
    conv_f3(ops, cfg, FUSION, 1, True)


@pytest.mark.parametrize("cfg", [-1, 7, 10, 13, 104, 134, 164])
def test_f3_conv_row_vector_slice_splitk(ops, cfg):
    conv_f3(ops, cfg, SPLIT_SM if cfg >= 100 else SPLIT_TILED, 3, False)


# ------------------------------------------------------------------------------------------------ F4: column slices
@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("fam", FAMILIES, ids=ids(FAMILIES))
def test_f4_column_slices(ops, fam, out_f32):
    m, n, (k1, k2), rpbs = fam.shape
    p, acc = problem(fam, rpbs[0])
    want = X.round_once(X.epilogue(acc, p.bias, res=p.res), out_f32)
    a, w, bias = X.dev(p.a), X.dev(p.w), X.dev32(p.bias)
    for name, (opad, ooff, rpad, roff) in SLICES.items():
        obuf, out = sliced(torch.empty(m, n, dtype=want.dtype, device="cuda"), opad, ooff, X.sentinel(want.dtype))
        out[:] = X.sentinel(want.dtype).cuda()
        before = obuf.clone()
        _, res = sliced(X.dev(p.res), rpad, roff, NAN)
        attempt(ops, fam, "F4", lambda: launch(ops, fam, a, w, False, bias=bias, res=res, out=out, out_f32=out_f32), obuf)
        check_route(ops, fam)
        X.assert_same_bits(out, want, f"{fam.id} F4 {name}: out = columns [{ooff}, {ooff + n}) of [m][{n + opad}], ldres {n + rpad}")
        assert X.outside_unchanged(obuf, before, ooff, n), f"{fam.id} F4 {name}: the guard columns of out were written"


# ------------------------------------------------------------------------------------------------ F5: GEGLU
@pytest.mark.parametrize("c", X.GEGLU_GATES)
@pytest.mark.parametrize("fam", GEGLU_FAMILIES, ids=ids(GEGLU_FAMILIES))
def test_f5_geglu_packed_weight_and_wide_output(ops, fam, c):
    from mvd_amd.packing import _geglu_rows
    m, n_out, k = GEGLU
    a64, w64, bias64, _, want = X.geglu_problem(m, n_out, k, c)
    a, w, bias = X.dev(a64), X.dev(_geglu_rows(w64)), X.dev32(_geglu_rows(bias64))
    opad, ooff = EVEN[:2]
    obuf, out = sliced(torch.empty(m, n_out, dtype=torch.bfloat16, device="cuda"), opad, ooff, X.sentinel(torch.bfloat16))
    out[:] = X.sentinel(torch.bfloat16).cuda()
    before = obuf.clone()
    if attempt(ops, fam, "F5", lambda: launch(ops, fam, a, w, True, bias=bias, geglu=True, out=out), obuf) is None:
        return
    check_route(ops, fam, (m, 2 * n_out, k, True))
    one_ulp, few, text = X.geglu_ok(out.cpu().contiguous(), want)
    assert one_ulp and few, f"{fam.id} F5, gate {c}: {text}"
    assert X.outside_unchanged(obuf, before, ooff, n_out), f"{fam.id} F5: the guard columns of out were written"


# ------------------------------------------------------------------------------------------------ F1 + F3 + F4
@pytest.mark.parametrize("fam", FAMILIES, ids=ids(FAMILIES))
def test_all_forms_together(ops, fam):
    m, n, (k1, k2), rpbs = fam.shape
    rpb = rpbs[-1]
    p, acc = problem(fam, rpb)
    a, w, bias = X.dev(p.a), X.dev(p.w), X.dev32(p.bias)
    rv = X.dev32(rowvec_buffer(p.rowvec))[:, n:2 * n] if rpb else None
    opad, ooff, rpad, roff = EVEN
    for alpha in X.ALPHAS + ("in place",):
        inplace = alpha == "in place"
        al = 1.0 if inplace else alpha
        want = X.round_once(X.epilogue(acc, p.bias, p.rowvec, rpb, p.res, al))
        if inplace:
            obuf, out = sliced(X.dev(p.res), opad, ooff, X.sentinel(torch.bfloat16))
            res = out
        else:
            obuf, out = sliced(torch.empty(m, n, dtype=torch.bfloat16, device="cuda"), opad, ooff, X.sentinel(torch.bfloat16))
            out[:] = X.sentinel(torch.bfloat16).cuda()
            _, res = sliced(X.dev(p.res), rpad, roff, NAN)
        before = obuf.clone()
        got = attempt(ops, fam, "ALL", lambda: launch(ops, fam, a, w, True, bias=bias, rowvec=rv, rows_per_batch=rpb, res=res, out=out, alpha=al), obuf)
        if got is None:
            continue
        check_route(ops, fam)
        X.assert_same_bits(out, want, f"{fam.id} ALL alpha {alpha}")
        assert X.outside_unchanged(obuf, before, ooff, n), f"{fam.id} ALL alpha {alpha}: the guard columns of out were written"


# ------------------------------------------------------------------------------------------------ refusals of the launchers
MISALIGNED = [_fam("cfg-1", EPI, force_cfg=-1), _fam("cfg7", EPI, force_cfg=7), _fam("sm0", EPI, force_cfg=sm_cfg(0)),
              _fam("split3_cfg-1", SPLITK, force_cfg=-1, splitk=3), _fam("sm0_split2", SM_SPLITK, force_cfg=sm_cfg(0), splitk=2)]


@pytest.mark.parametrize("fam", MISALIGNED, ids=ids(MISALIGNED))
def test_misaligned_row_vector_is_refused(ops, fam):
    """Every family reads the row vector as f32x4: a base 4 bytes off a 16-byte boundary, or a row stride that is no multiple of
    4 floats, is refused on the host (mvd_launch_gemm, mvd_launch_gemm_sm) -- and the output stays untouched."""
    from mvd_amd._lib import MvdError
    m, n, (k1, k2), rpbs = fam.shape
    rpb = rpbs[-1]
    p, _ = problem(fam, rpb)
    a, w, bias = X.dev(p.a), X.dev(p.w), X.dev32(p.bias)
    base_off = X.dev32(rowvec_buffer(p.rowvec))[:, n + 1:2 * n + 1]
    bad_stride = X.embed(X.dev32(p.rowvec), n + 2, 0, 0.0)[:, :n]
    for what, rv in (("base", base_off), ("stride", bad_stride)):
        out = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
        out[:] = X.sentinel(torch.bfloat16).cuda()
        before = out.clone()
        with pytest.raises(MvdError, match="row vector"):
            ops.linear_ld(a, w, bias, rowvec=rv, rows_per_batch=rpb, out=out, **fam.kw)
        torch.cuda.synchronize()
        assert X.outside_unchanged(out, before, 0, 0), f"{fam.id}: misaligned {what}, refused, but the output was written"


def test_misaligned_conv_row_vector_is_refused(ops):
    from mvd_amd._lib import MvdError
    B, H, W, cin, cout = SPLIT_TILED
    p = X.conv_problem(*SPLIT_TILED)
    rv = X.dev32(rowvec_buffer(p.rowvec))[:, cout + 1:2 * cout + 1]
    for cfg in (-1, sm_cfg(0, 4)):
        with pytest.raises(MvdError, match="row vector"):
            ops.conv3x3(X.dev(p.x), X.dev(TC.pack(p.w)), X.dev32(p.bias), rowvec=rv, force_cfg=cfg)
