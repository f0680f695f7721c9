"""Bit-exact GEMM tests: every GEMM form (gemm.hip, gemm_pp.hip, gemm_sm.hip, gemm_xs.hip) on the integer problems of
exact_util.py, compared bitwise with the fp64 reference rounded once to bf16.  One wrong k element, one element on a split-K
slab boundary, a wrong row-vector row or a wrong rounding of a tie fails these; the tolerance tests of test_ops_gpu.py cannot
see any of them.  The GEGLU forms go through an approximate gelu (common.h, |err| <= 1.5e-7): there no element may be more than
one bf16 ulp off and at most 1 % may differ at all, which still pins the value / gate row interleave exactly."""
import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

# the suite's own GEMM shapes (test_ops_gpu.py), the tile configs of test_linear_configs and their tile widths
SHAPES = [(300, 640, 320), (1024, 1280, 192), (77, 640, 1024), (5, 1920, 64), (2100, 320, 128)]
CFGS = [-1, 2, 3, 4, 5, 7, 10, 11, 12, 13]
TILE_N = {2: 160, 3: 128, 4: 64, 5: 64, 7: 320, 6: 320}
PERSISTENT = (8500, 2560, 64)                 # 34 x 8 tiles of 256x320 on a grid of 256 workgroups: a second pass, ragged rows
EPI = (384, 640, 128, 192)                    # m, n, k1, k2 of the epilogue cases; rows_per_batch 128 (inside a tile) / 96 (straddles)
EPI_RPB = (128, 96)
SPLITK = (100, 320, 640, 50)                  # m, n, k, rows_per_batch: separate reduce (tiled kernels)
SM_SPLITK = (200, 640, 640, 100)              # in-kernel combine (small-M kernels)
NOWAIT = (1024, 1280, 1536, 12)               # the no-wait combine of test_ops_gpu.py
SM_BN = {0: 64, 1: 64, 2: 128, 3: 128, 4: 160, 5: 160, 6: 320}
XS_K = 320
XS_SHAPES = [(77, 320), (1000, 640), (4129, 1280)]
GEGLU = (300, 1280, 320)                      # m, output width (the GEMM's N is twice that), k
GEGLU_CFGS = [-1, 3, 4, 5, 6, 11, 12, 13]
GEGLU_SM_TILES = [0, 1, 2, 3, 6]

CFG_CASES = [(c, m, n, k) for c in CFGS for (m, n, k) in SHAPES if c < 0 or n % TILE_N[c % 8] == 0]
SM_CASES = [(t, m, n, k) for t in range(7) for (m, n, k) in SHAPES if n % SM_BN[t] == 0]
XS_CASES = [(cs, m, n) for cs in (0, 1, 2) for (m, n) in XS_SHAPES if cs == 0 or (n // 64) % cs == 0]


def gemm_shapes():
    """(m, n, k, rowvec groups) of every integer GEMM problem this file runs (test_exact_inputs_cpu.py checks the generators on them)"""
    out = [(m, n, k, 0) for (m, n, k) in SHAPES] + [PERSISTENT + (0,)]
    out += [(EPI[0], EPI[1], EPI[2] + EPI[3], EPI[0] // r) for r in EPI_RPB]
    out += [(SPLITK[0], SPLITK[1], SPLITK[2], SPLITK[0] // SPLITK[3]), (SM_SPLITK[0], SM_SPLITK[1], SM_SPLITK[2], SM_SPLITK[0] // SM_SPLITK[3])]
    out += [NOWAIT[:3] + (0,)] + [(m, n, XS_K, 0) for (m, n) in XS_SHAPES]
    return out


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def sm_cfg(tile, depth):
    return 100 + 10 * tile + depth


def both_layouts(ops, p_w, run):
    """run(w, blocked) for the plain weight and for packing.block_weight of it: identical results, returned once"""
    from mvd_amd.packing import block_weight
    w = X.dev(p_w)
    plain = run(w, None)
    blocked = run(block_weight(w), tuple(w.shape))
    X.assert_same_bits(blocked, plain.cpu(), "blocked weight layout vs plain")
    return plain


# ------------------------------------------------------------------------------------------------ dense, bias only
@pytest.mark.parametrize("cfg,m,n,k", CFG_CASES)
def test_linear_configs_exact(ops, cfg, m, n, k):
    p = X.gemm_problem(m, n, k)
    want = X.round_once(X.epilogue(X.gemm_acc(m, n, k), p.bias))
    got = ops.linear(X.dev(p.a), X.dev(p.w), X.dev32(p.bias), force_cfg=cfg)
    X.assert_same_bits(got, want, f"linear cfg {cfg} {m}x{n}x{k}")


def test_linear_persistent_second_pass_exact(ops):
    """More 256x320 tiles than workgroups: the tiles a workgroup takes on its second pass, the last of them ragged."""
    m, n, k = PERSISTENT
    p = X.gemm_problem(m, n, k)
    got = ops.linear(X.dev(p.a), X.dev(p.w), X.dev32(p.bias))
    plan = ops.last_gemm_plan()
    ok = plan["cfg"] == 7 and plan["tiles"] > plan["grid"]
    assert ok, plan
    X.assert_same_bits(got, X.round_once(X.epilogue(X.gemm_acc(m, n, k), p.bias)), "persistent 256x320")


def epilogue_variants(ops, cfg, run_w):
    """dual source a | a2, row vector (rows_per_batch inside / straddling a tile), residual, alpha, each alone and all together;
    fp32 output.  run_w(w64, f): f(w, blocked) launches with a device weight -- plain, or both layouts for the small-M kernels."""
    m, n, k1, k2 = EPI
    for rpb in EPI_RPB:
        p = X.gemm_problem(m, n, k1 + k2, m // rpb)
        acc = X.gemm_acc(m, n, k1 + k2, m // rpb)
        a, a2, bias, rowvec, res = X.dev(p.a[:, :k1]), X.dev(p.a[:, k1:]), X.dev32(p.bias), X.dev32(p.rowvec), X.dev(p.res)
        full = X.dev(p.a)
        singles = [dict(rowvec=True), dict(res=True), dict(alpha=0.5), dict(alpha=2.0), dict(dual=True)]
        for v in singles + [dict(dual=True, rowvec=True, res=True, alpha=al) for al in X.ALPHAS]:
            alpha = v.get("alpha", 1.0)
            want = X.round_once(X.epilogue(acc, p.bias, p.rowvec if v.get("rowvec") else None, rpb, p.res if v.get("res") else None, alpha))
            kw = dict(alpha=alpha, force_cfg=cfg)
            if v.get("rowvec"):
                kw.update(rowvec=rowvec, rows_per_batch=rpb)
            if v.get("res"):
                kw.update(res=res)
            if v.get("dual"):
                got = run_w(p.w, lambda w, blk: ops.linear(a, w, bias, a2=a2, blocked=blk, **kw))
            else:
                got = run_w(p.w, lambda w, blk: ops.linear(full, w, bias, blocked=blk, **kw))
            X.assert_same_bits(got, want, f"linear cfg {cfg} rows_per_batch {rpb} {v}")
    want32 = X.round_once(X.epilogue(acc, p.bias, alpha=0.5), out_f32=True)
    got32 = run_w(p.w, lambda w, blk: ops.linear(full, w, bias, alpha=0.5, out_f32=True, force_cfg=cfg, blocked=blk))
    X.assert_same_bits(got32, want32, f"linear cfg {cfg} fp32 out")


@pytest.mark.parametrize("cfg", CFGS)
def test_linear_epilogues_exact(ops, cfg):
    epilogue_variants(ops, cfg, lambda w64, f: f(X.dev(w64), None))


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("splitk", [2, 3, 5])
@pytest.mark.parametrize("cfg", [-1, 7, 10, 13])
def test_linear_splitk_separate_reduce_exact(ops, cfg, splitk):
    m, n, k, rpb = SPLITK
    p = X.gemm_problem(m, n, k, m // rpb)
    for alpha in X.ALPHAS:
        want = X.round_once(X.epilogue(X.gemm_acc(m, n, k, m // rpb), p.bias, p.rowvec, rpb, p.res, alpha))
        got = ops.linear(X.dev(p.a), X.dev(p.w), X.dev32(p.bias), rowvec=X.dev32(p.rowvec), rows_per_batch=rpb, res=X.dev(p.res),
                         alpha=alpha, force_cfg=cfg, splitk=splitk)
        X.assert_same_bits(got, want, f"linear cfg {cfg} split-K {splitk} alpha {alpha}")


@pytest.mark.parametrize("splitk", [2, 3, 5])
@pytest.mark.parametrize("tile", [0, 1, 3, 5, 6])
def test_sm_splitk_in_kernel_combine_exact(ops, tile, splitk):
    m, n, k, rpb = SM_SPLITK
    p = X.gemm_problem(m, n, k, m // rpb)
    a, bias, rowvec, res = X.dev(p.a), X.dev32(p.bias), X.dev32(p.rowvec), X.dev(p.res)
    for alpha in X.ALPHAS:
        want = X.round_once(X.epilogue(X.gemm_acc(m, n, k, m // rpb), p.bias, p.rowvec, rpb, p.res, alpha))
        got = both_layouts(ops, p.w, lambda w, blk: ops.linear(a, w, bias, rowvec=rowvec, rows_per_batch=rpb, res=res, alpha=alpha,
                                                              force_cfg=sm_cfg(tile, 3), splitk=splitk, blocked=blk))
        X.assert_same_bits(got, want, f"sm tile {tile} split-K {splitk} alpha {alpha}")


def test_sm_splitk_nowait_combine_exact(ops):
    m, n, k, splitk = NOWAIT
    p = X.gemm_problem(m, n, k)
    got = ops.linear(X.dev(p.a), X.dev(p.w), X.dev32(p.bias), force_cfg=sm_cfg(0, 4), splitk=splitk)
    plan = ops.last_gemm_plan()
    ok = plan["grid"] == 16 * 20 * splitk and plan["nowait"] == 1
    assert ok, plan
    X.assert_same_bits(got, X.round_once(X.epilogue(X.gemm_acc(m, n, k), p.bias)), "sm no-wait combine")


# ------------------------------------------------------------------------------------------------ small-M kernels
@pytest.mark.parametrize("depth", [2, 3, 4, 8])
@pytest.mark.parametrize("tile,m,n,k", SM_CASES)
def test_sm_linear_exact_plain_and_blocked(ops, tile, depth, m, n, k):
    p = X.gemm_problem(m, n, k)
    a, bias = X.dev(p.a), X.dev32(p.bias)
    got = both_layouts(ops, p.w, lambda w, blk: ops.linear(a, w, bias, force_cfg=sm_cfg(tile, depth), blocked=blk))
    X.assert_same_bits(got, X.round_once(X.epilogue(X.gemm_acc(m, n, k), p.bias)), f"sm tile {tile} depth {depth} {m}x{n}x{k}")


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6])
def test_sm_linear_epilogues_exact(ops, tile):
    epilogue_variants(ops, sm_cfg(tile, 3), lambda w64, f: both_layouts(ops, w64, f))


# ------------------------------------------------------------------------------------------------ X-stationary kernel
@pytest.mark.parametrize("csplit,m,n", XS_CASES)
def test_xs_exact(ops, csplit, m, n):
    """K = 320: bias (integers are exact in the hi + lo split), residual, ragged M, operands that are column slices of wider buffers"""
    from mvd_amd.packing import pack_xs
    p = X.gemm_problem(m, n, XS_K)
    acc = X.gemm_acc(m, n, XS_K)
    x, res = X.dev(p.a), X.dev(p.res)
    wp, wp0 = pack_xs(X.f32(p.w), X.f32(p.bias)).cuda(), pack_xs(X.f32(p.w), None).cuda()
    X.assert_same_bits(ops.linear_xs(x, wp, csplit=csplit), X.round_once(X.epilogue(acc, p.bias)), "xs bias")
    X.assert_same_bits(ops.linear_xs(x, wp0, csplit=csplit), X.round_once(acc), "xs no bias")
    want = X.round_once(X.epilogue(acc, p.bias, res=p.res))
    X.assert_same_bits(ops.linear_xs(x, wp, res=res, csplit=csplit), want, "xs residual")
    xbig = torch.full((m, 3 * XS_K), 3.0, device="cuda", dtype=torch.bfloat16)
    rbig = torch.full((m, 2 * n), 5.0, device="cuda", dtype=torch.bfloat16)
    xbig[:, XS_K:2 * XS_K] = x
    rbig[:, n:] = res
    got = ops.linear_xs(xbig[:, XS_K:2 * XS_K], wp, res=rbig[:, n:], csplit=csplit)
    X.assert_same_bits(got, want, "xs strided operands")


# ------------------------------------------------------------------------------------------------ GEGLU
def geglu_case(c, launch, what):
    from mvd_amd.packing import _geglu_rows
    m, n_out, k = GEGLU
    a, w, bias, _, want = X.geglu_problem(m, n_out, k, c)
    got = launch(X.dev(a), _geglu_rows(w), _geglu_rows(bias), w, bias).cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    one_ulp, few, text = X.geglu_ok(got, want)
    assert one_ulp and few, f"{what}, gate {c}: {text}"


@pytest.mark.parametrize("c", X.GEGLU_GATES)
@pytest.mark.parametrize("cfg", GEGLU_CFGS)
def test_linear_geglu_interleave(ops, cfg, c):
    geglu_case(c, lambda a, wr, br, w, b: ops.linear(a, X.dev(wr), X.dev32(br), geglu=True, force_cfg=cfg), f"geglu cfg {cfg}")


@pytest.mark.parametrize("c", X.GEGLU_GATES)
@pytest.mark.parametrize("tile", GEGLU_SM_TILES)
def test_sm_geglu_interleave_plain_and_blocked(ops, tile, c):
    geglu_case(c, lambda a, wr, br, w, b: both_layouts(ops, wr, lambda wd, blk: ops.linear(a, wd, X.dev32(br), geglu=True,
                                                                                        force_cfg=sm_cfg(tile, 3), blocked=blk)),
               f"sm geglu tile {tile}")


@pytest.mark.parametrize("c", X.GEGLU_GATES)
def test_xs_geglu_interleave(ops, c):
    from mvd_amd.packing import pack_xs
    geglu_case(c, lambda a, wr, br, w, b: ops.linear_xs(a, pack_xs(X.f32(w), X.f32(b), geglu=True).cuda(), geglu=True), "xs geglu")
