"""Spike probes of the kernels that compute a statistic (inputs, references and the two-tier check: stat_probe.py).

Every case asserts its ROUTE first, from the plan the library records -- ops.last_groupnorm_plan() for GroupNorm (the expected
plan is part of the case: the hot positions of a large domain are built from it, and the CPU file has to enumerate them without a
GPU), ops.last_gemm_plan() for the LayerNorm folds -- and then runs its launches against the fp64 reference.  A case's launches
share one device-resident background; references run in torch fp64 on the device.  ln_kernel has no plan hook: its
instantiation <1, 2, 4> follows from c alone (c <= 512, <= 1024, above), and the case list has partly filled and full last vectors
of each.  Each test prints its launches, the positions probed and the worst error of either tier as a fraction of the 2^-7 limit.

The GEGLU forms of the folds multiply LayerNorm(x) by gelu(c) of a constant gate (zero gate weights, bias c, as
exact_util.geglu_problem does): for them only, the hot tier is 2^-7 + 1.5e-7 / |gelu(c)| -- the |error| <= 1.5e-7 that
csrc/common.h documents for gelu_erf_f, relative to the factor it perturbs (the reasoning of exact_util.geglu_ok)."""
import pytest
import torch

import stat_probe as P

pytestmark = pytest.mark.gpu

GROUPS = 32
SLICE = lambda nv, threads, gpw, npl: dict(form="slice", nv=nv, threads=threads, gpw=gpw, npl=npl)                      # noqa: E731
TWO = lambda R, nchunk, rpc, apply_rows: dict(form="two_kernel", R=R, threads=256, nchunk=nchunk, rows_per_chunk=rpc,   # noqa: E731
                                              apply_rows=apply_rows)

# (name, batch, hw, c0, c1, background shift, DebugFlag.GN_ONE_PASS, expected plan).  The plan is what the launcher reports for
# the shape TODAY: the hot positions of the large domains are built from it, and the CPU file enumerates them without a GPU.  A
# retuned launcher fails the plan assertion of these tests -- then bring the case's plan up to date; the kernel is not suspect.
GN_SLICE_CASES = [
    # C = 320: cg 10, four groups per slice, a thread's vector straddles two groups
    ("nv2", 2, 64, 320, 0, 0.0, False, SLICE(2, 256, 4, 51)),
    ("nv4", 3, 200, 320, 0, 0.0, False, SLICE(4, 256, 4, 51)),
    ("nv8-ragged-batch8", 8, 1000, 320, 0, 0.0, False, SLICE(8, 1024, 4, 204)),      # batch % 8 == 0: XCD-swizzled block order
    ("nv16-ragged", 16, 3001, 320, 0, 0.0, False, SLICE(16, 1024, 4, 204)),          # the smallest batch the launcher accepts
    ("nv21-batch1", 1, 4096, 320, 0, 0.0, True, SLICE(21, 1024, 4, 204)),
    ("two-source-straddle", 2, 64, 640, 320, 0.0, False, SLICE(4, 256, 4, 17)),      # cg 30: group 21 holds channels of both sources
    ("two-source-edge", 3, 64, 320, 320, 0.0, False, SLICE(2, 256, 2, 51)),          # cg 20: c0 is a group edge
]
GN_TWO_CASES = [
    ("c64", 2, 256, 64, 0, 0.0, False, TWO(32, 32, 8, 32)),                          # cg 2
    ("c128-ragged", 1, 100, 128, 0, 0.0, False, TWO(16, 12, 9, 16)),                 # cg 4, a ragged last chunk
    # The batch-1 cases have 32 domains per launch, 1024 slots in BUDGET launches: fewer than must-hit pixels x channels.  Each
    # must-hit pixel keeps ONE channel index (cycling over the pixels), and 64x64x320 keeps 1024 of its 1491 pixels -- the edges of
    # the apply kernel's blocks go last.  TRUNCATED names them; every other case must hold its full list (asserted).
    ("batch1-64x64x320", 1, 4096, 320, 0, 0.0, False, TWO(6, 64, 64, 7)),
    ("ragged-1296", 1, 1296, 640, 0, 0.0, False, TWO(3, 62, 21, 4)),
    ("ragged-1296-mean60", 1, 1296, 640, 0, 60.0, False, TWO(3, 62, 21, 4)),
    ("two-source-1296", 1, 1296, 640, 320, 0.0, False, TWO(2, 62, 21, 3)),
]
TRUNCATED = {"batch1-64x64x320", "ragged-1296", "ragged-1296-mean60", "two-source-1296"}
FILL_LAUNCHES = 8           # a large domain gets at least this many launches (a truncated one the whole budget): seeded interior
                            # pixels behind the must-hit list
LN_C = [64, 320, 512, 640, 1024, 1280, 2048]
REFNORM_CASES = [(3, 960, 320), (32, 64, 64)]
GEGLU_GATE = 1.0
# (kernel, K, M, GEGLU, expected tile config: 9 = X-stationary, 100.. = small-M, 7 / 6 = ping-pong)
FOLD_CASES = [
    ("xs", 320, 77, False, 9), ("xs", 320, 1000, False, 9), ("xs", 320, 1000, True, 9),
    ("sm", 320, 653, False, 100), ("sm", 640, 1293, False, 100), ("sm", 1280, 2573, False, 100), ("sm", 320, 653, True, 100),
    # the smallest M the launcher gives to the 256x320 ping-pong kernel: 200 tiles (N = K: ceil(M / 256) * K / 320 >= 200)
    ("pp", 320, 199 * 256 + 1, False, 7), ("pp", 640, 99 * 256 + 1, False, 7), ("pp", 320, 99 * 256 + 1, True, 6),
]


def case_id(c):
    return c[0] if isinstance(c[0], str) and len(c) == 8 else "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------ what a case probes (CPU side)
def gn_probe(case):
    """(layout, must-hit entries, info, schedule) of a GroupNorm case -- pure, shared with test_stat_probe_cpu.py"""
    name, B, hw, c0, c1, shift, flag, plan = case
    lay = P.GN(B, hw, c0 + c1, GROUPS)
    if lay.n <= P.EXHAUSTIVE_MAX:
        # (two sources: the channels either side of c0 are bound to the groups that own them, ahead of all the positions)
        bound = tuple(e for e in P.must_hit(plan, hw, lay.cg, c0 if c1 else 0)[0] if e[0] >= 0)
        must, info = bound + P.exhaustive(lay.n), dict(exhaustive=True)
    else:
        must, info = P.must_hit(plan, hw, lay.cg, c0 if c1 else 0, capacity=P.BUDGET * lay.ndom)
    assert info.get("full", True) == (name not in TRUNCATED), (name, info)
    launches = 0 if lay.n <= P.EXHAUSTIVE_MAX else P.BUDGET if name in TRUNCATED else FILL_LAUNCHES
    return lay, must, info, P.schedule(lay.n, lay.ndom, must, GROUPS, seed=hw + c0, cg=lay.cg, launches=launches)


def gn_affine(C):
    g = torch.Generator().manual_seed(C)
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def ln_affine(c):
    g = torch.Generator().manual_seed(c + 1)
    return 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)


def ln_hot(rows, c, step=0):
    return (torch.arange(rows) + step) % c


def refnorm_probe(case):
    B, hw, c = case
    lay = P.RefNorm(B, hw, c)
    return lay, P.schedule(lay.n, lay.ndom, P.exhaustive(lay.n), 1, seed=B)


def fold_affine(k):
    """bf16-exact, different per column: the folded weight diag(gamma) and the constants c1 = gamma, c2 = beta are exact"""
    j = torch.arange(k)
    return 1 + (j % 8).float() / 8, ((j % 5).float() - 2) / 4


def fold_slots(k, m):
    """(launches, M): hot column = (row + launch * step) mod K.  Every column is hot in at least two rows of different 16-row
    MFMA tiles and of different row index mod 16 (another lane of the fragment): M >= 2 K has rows K apart in one launch -- same
    lane -- so a second launch shifts by 7; a short M walks the columns in steps of M (odd), twice round and once more."""
    steps = [0, 7] if m >= 2 * k else [i * m for i in range(3 * -(-k // m))]
    return torch.stack([ln_hot(m, k, st) for st in steps])


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def report(what, launches, positions, worst):
    print(f"\n[stat-probe] {what}: {launches} launches, {positions} positions probed, worst hot {worst[0]:.3f}, "
          f"worst non-hot {worst[1]:.3f} of the limit")


def run(lay, bg, slots, launch, reference, what, hot_tol=P.TOL):
    worst = [0.0, 0.0]
    for i in range(len(slots)):
        hot = slots[i].cuda()
        x = P.with_spike(bg, hot)
        got = launch(x, i)
        r = P.check(lay.to_dom(got), reference(x), hot, lay, f"{what}, launch {i}", hot_tol)
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    report(what, len(slots), slots.numel(), worst)


# ------------------------------------------------------------------------------------------------ GroupNorm
def _groupnorm(ops, case, silu):
    from mvd_amd import _lib as L
    name, B, hw, c0, c1, shift, flag, plan = case
    lay, must, info, slots = gn_probe(case)
    bg = P.background(lay.ndom, lay.n, hw + c0, shift).cuda()
    gamma, beta = gn_affine(c0 + c1)
    gam, bet = (t.cuda() for t in lay.affine(gamma, beta))
    gamma, beta = gamma.cuda(), beta.cuda()

    def launch(x, i):
        full = lay.from_dom(x)
        x0 = full[..., :c0].contiguous() if c1 else full
        x1 = full[..., c0:].contiguous() if c1 else None
        if flag:
            L.lib().mvd_debug_set_flags(L.DebugFlag.GN_ONE_PASS)
        try:
            got = ops.groupnorm(x0, gamma, beta, GROUPS, 1e-5, silu, x2=x1)
        finally:
            if flag:
                L.lib().mvd_debug_set_flags(0)
        got_plan = ops.last_groupnorm_plan()
        assert got_plan == plan, (f"{name}: the launcher reports {got_plan}, the case expects {plan}.  If the launcher was retuned, "
                                  "update the case's plan in GN_*_CASES (the hot positions follow from it); the kernel is not suspect.")
        return got

    run(lay, bg, slots, launch, lambda x: P.reference(x, 1e-5, gam, bet, silu), f"groupnorm {name} silu={silu} {plan} {info}")


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case", GN_SLICE_CASES, ids=case_id)
def test_groupnorm_slice_kernel(ops, case, silu):
    _groupnorm(ops, case, silu)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case", GN_TWO_CASES, ids=case_id)
def test_groupnorm_two_kernel_form(ops, case, silu):
    _groupnorm(ops, case, silu)


# ------------------------------------------------------------------------------------------------ LayerNorm, reference normalisation
@pytest.mark.parametrize("c", LN_C)
def test_layernorm(ops, c):
    """rows = c + 3 (ragged against four rows per block), hot column = row mod c: one launch is exhaustive"""
    rows = c + 3
    lay = P.Rows(rows, c)
    gamma, beta = ln_affine(c)
    gam, bet = (t.cuda() for t in lay.affine(gamma, beta))
    gamma, beta = gamma.cuda(), beta.cuda()
    run(lay, P.background(rows, c, c).cuda(), ln_hot(rows, c)[None], lambda x, i: ops.layernorm(x, gamma, beta),
        lambda x: P.reference(x, 1e-5, gam, bet), f"layernorm {rows}x{c}")


@pytest.mark.parametrize("case", REFNORM_CASES, ids=case_id)
def test_refnorm(ops, case):
    lay, slots = refnorm_probe(case)
    run(lay, P.background(lay.ndom, lay.n, case[0]).cuda(), slots, lambda x, i: ops.refnorm(lay.from_dom(x)),
        P.refnorm_reference, f"refnorm {case}")


# ------------------------------------------------------------------------------------------------ LayerNorm folds in the GEMMs
@pytest.mark.parametrize("case", FOLD_CASES, ids=case_id)
def test_layernorm_fold(ops, case):
    """Identity weight (N = K), no bias: the output row is LayerNorm(x) itself (GEGLU: times gelu of the constant gate)."""
    from mvd_amd._lib import MvdError
    from mvd_amd.packing import _geglu_rows, fold_layernorm, pack_xs
    kernel, k, m, geglu, cfg = case
    lay = P.Rows(m, k)
    gamma, beta = fold_affine(k)
    gam, bet = (t.cuda() for t in lay.affine(gamma, beta))
    w, bias = torch.eye(k), None
    if geglu:
        w = torch.cat([w, torch.zeros(k, k)], 0)
        bias = torch.cat([torch.zeros(k), torch.full((k,), GEGLU_GATE)], 0)
    if kernel == "xs":
        wf, cf = fold_layernorm(w, gamma, beta, bias, "cpu")
        wp = pack_xs(wf.float(), cf[1], geglu=geglu).cuda()
        op = lambda x: ops.linear_xs(x, wp, geglu=geglu, ln=True)                                     # noqa: E731
    else:
        wf, cf = fold_layernorm(_geglu_rows(w), gamma, beta, _geglu_rows(bias), "cuda") if geglu else fold_layernorm(w, gamma, beta, None, "cuda")
        op = lambda x: ops.ln_linear(x, wf, cf, geglu=geglu)                                          # noqa: E731

    def launch(x, i):
        got = op(x)
        plan = ops.last_gemm_plan()
        assert plan["cfg"] == cfg or (cfg == 100 and 100 <= plan["cfg"] < 200), (case, plan)
        return got

    if kernel == "pp":          # M is the smallest the ping-pong fold takes: one row fewer has no fused kernel at all
        with pytest.raises(MvdError):
            op(torch.zeros(m - 1, k, device="cuda", dtype=torch.bfloat16))
    scale = P.gelu64(GEGLU_GATE) if geglu else 1.0
    hot_tol = P.TOL + (P.GELU_ERR / abs(scale) if geglu else 0.0)
    slots = fold_slots(k, m)
    run(lay, P.background(m, k, k + m).cuda(), slots, launch, lambda x: P.reference(x, 1e-5, gam, bet, scale=scale),
        f"ln-fold {kernel} K={k} M={m} geglu={geglu}", hot_tol)
