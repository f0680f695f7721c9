"""Token merging on the CPU: the margin the GPU operator tests compare scores with, the ambiguity count of
every seeded input of tests/test_tome_ops_gpu.py, the proof that the GPU file's checks catch the op-level faults (run on a CPU
emulation of the operators, ``tome_ref.emulate``), and the separation study that the engine parity bound rests on."""
import functools

import pytest
import torch

from tests import tome_ref as T


# ------------------------------------------------------------------------------------------------------------- the margin
@pytest.mark.parametrize("C", [64, 320, 640, 1280])
def test_margin_holds_for_fp32_sums_in_any_order(C):
    """scores from exact products added in fp32 one at a time in shuffled orders (and a pairwise order), divided by fp32 norms, stay
    within tau / 2 of the fp64 score; tau is 4 (C + 4) 2^-24 (``tome_ref.tau`` derives it)"""
    assert T.tau(C) == 4 * (C + 4) * 2.0 ** -24
    H = W = 6
    x = T.seeded_map(2, H, W, C, 3)
    want = T.scores(x, H, W).max(dim=-1).values
    g = torch.Generator().manual_seed(C)
    worst = 0.0
    for trial in range(4):
        perm = None if trial == 0 else torch.randperm(C, generator=g)
        got = T.emulate(x, H, W, 9, perm=perm)["score"]
        worst = max(worst, (got.double() - want).abs().max().item())
    # a different association: fp32 pairwise sums (torch's reduction)
    dst, src = T.geometry(H, W)
    xf = x.float()
    pair = (xf[:, src] @ xf[:, dst].transpose(1, 2)) / (xf[:, src].norm(dim=-1)[:, :, None] * xf[:, dst].norm(dim=-1)[:, None, :])
    worst = max(worst, (pair.max(dim=-1).values.double() - want).abs().max().item())
    print(f"C = {C}: largest fp32 score error {worst:.3e}, tau / 2 = {T.tau(C) / 2:.3e}")
    assert worst <= T.tau(C) / 2


def test_products_of_bf16_are_exact_in_fp32():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(4096, generator=g).to(torch.bfloat16), torch.randn(4096, generator=g).to(torch.bfloat16)
    assert torch.equal((a.float() * b.float()).double(), a.double() * b.double())


# -------------------------------------------------------------------------------------------------------------- ambiguity
@pytest.mark.parametrize("case", T.SMALL_CASES + T.LARGE_CASES, ids=T.case_id)
def test_reference_ambiguity_of_every_gpu_case(case):
    """zero ambiguous src at the small shapes, inside the 2 % cap at the two large ones"""
    (B, H, W, C, r), seed = case
    x = T.seeded_map(B, H, W, C, seed)
    sc = T.scores(x, H, W)
    n = int(T.ambiguous(sc, r, T.tau(C)).sum())
    print(f"{T.case_id(case)}: {n} ambiguous src of {B * sc.shape[1]}")
    if case in T.SMALL_CASES:
        assert n == 0
    assert n <= T.AMBIGUOUS_CAP * B * sc.shape[1]


def test_the_planted_ties_case_is_well_posed():
    x, r, (d_lo, d_hi), (s_lo, s_hi) = T.planted_ties()
    dst, src = T.geometry(8, 8)
    assert torch.equal(x[:, dst[d_lo]], x[:, dst[d_hi]]) and torch.equal(x[:, src[s_lo]], x[:, src[s_hi]]) and d_lo < d_hi and s_lo < s_hi
    assert 0 < r < src.numel()
    o = T.emulate(x, 8, 8, r)
    T.check_planted_ties(x, 8, 8, r, ((d_lo, d_hi), (s_lo, s_hi)), o["best"], o["slot"])


# ------------------------------------------------------------------------------------------------------ op-level mutations
def _emulated(case, **wrong):
    (B, H, W, C, r), seed = case
    x = T.seeded_map(B, H, W, C, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    h_in = torch.randn(B, H * W, C, generator=g).to(torch.bfloat16)
    t_in = torch.randn(B, H * W - r, C, generator=g).to(torch.bfloat16)
    o = T.emulate(x, H, W, r, t_in=t_in, h_in=h_in, **wrong)
    return x, h_in, t_in, o


def _gpu_file_checks(case, x, h_in, t_in, o):
    (B, H, W, C, r), _ = case
    T.check_decisions(x, H, W, r, o["score"], o["best"], o["slot"])
    T.check_moves(x, o["slot"].clamp_min(0), H * W - r, o["merged"], h_in, t_in, o["h_out"])


@pytest.mark.parametrize("case", [T.SMALL_CASES[2], T.SMALL_CASES[1]], ids=T.case_id)
def test_the_emulation_passes_the_gpu_files_checks(case):
    _gpu_file_checks(case, *_emulated(case))


@pytest.mark.parametrize("wrong", [dict(dst_bottom_right=True), dict(drop_odd_row=True), dict(r_off=1), dict(r_off=-1), dict(use_sum=True),
                                   dict(neighbour_dst=True), dict(neighbour_row=True)], ids=lambda w: next(iter(w)) + str(next(iter(w.values()))))
def test_every_op_level_fault_fails_the_gpu_files_checks(wrong):
    """(2, 7, 9, 640, 17): odd both ways, so that a dropped last row shows"""
    case = T.SMALL_CASES[2]
    x, h_in, t_in, o = _emulated(case, **wrong)
    with pytest.raises(AssertionError):
        _gpu_file_checks(case, x, h_in, t_in, o)


def test_the_tie_to_the_higher_index_fails_the_planted_ties_check():
    x, r, dd, ss = T.planted_ties()
    o = T.emulate(x, 8, 8, r, tie_high=True)
    with pytest.raises(AssertionError):
        T.check_planted_ties(x, 8, 8, r, (dd, ss), o["best"], o["slot"])


def test_restatement_against_tomesd_when_it_is_installed():
    """tomesd is not a dependency; where it imports, its merge / unmerge with use_rand=False are the definition up to the row order"""
    tomesd = pytest.importorskip("tomesd")
    from tomesd.merge import bipartite_soft_matching_random2d
    B, H, W, C, r = 2, 8, 10, 64, 30
    x = T.seeded_map(B, H, W, C, 4).float()
    merge, unmerge = bipartite_soft_matching_random2d(x, W, H, 2, 2, r, no_rand=True)
    slot = T.reference_tables(x, H, W, r)
    mine = T.merge_rows(x, slot, H * W - r)
    theirs = merge(x, mode="mean")
    a = torch.randn(B, H * W - r, C)
    assert torch.allclose(torch.sort(theirs.flatten(1), dim=1).values, torch.sort(mine.flatten(1), dim=1).values, atol=1e-5)
    assert torch.allclose(T.unmerge(mine, slot), unmerge(theirs), atol=1e-5)
    del tomesd, a


# ----------------------------------------------------------------------------------------------- engine-level separation
@functools.lru_cache(maxsize=None)
def _oracle_setup():
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    cfg = OU.UNetConfig.tiny()
    return cfg, OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)


def _forward(inp):
    from oracle import mvd as OM
    cfg, params = _oracle_setup()
    with torch.no_grad():
        return OM.multiview_unet_forward(params, cfg, inp["sample"], torch.tensor(500), inp["text"], inp["src"], inp["tgt"], inp["lat"],
                                         fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)


@pytest.mark.parametrize("hw", [16, (16, 32)], ids=["16x16", "16x32"])
def test_parity_setting_tells_every_wrong_variant_apart(hw):
    """under ``tome_ref.PARITY_SETTING`` every wrong variant lies at least 4 x PARITY_BOUND_MAX from the ToMe oracle (tiny topology,
    the engine tests' inputs); measured 16 x 16: off 1.87e-1, attn2 merged 2.10e-1, the next level instead 2.00e-1, another row's
    table 2.15e-1, merged src left at zero 3.84e-1 -- so a cap of 3e-2 on the parity bound leaves a factor of six"""
    from tests.parity_util import make_inputs, rel_l2
    cfg, _ = _oracle_setup()
    inp = make_inputs(cfg, 2, hw, 7, 0, 96)
    plain = _forward(inp)
    rec = {}
    with T.tome_oracle(**T.PARITY_SETTING, record=rec):
        want = _forward(inp)
    assert sorted(rec) == ["down_block_0_attn_0", "down_block_0_attn_1", "up_block_3_attn_0", "up_block_3_attn_1", "up_block_3_attn_2"]
    with T.tome_oracle(**T.PARITY_SETTING, tables=rec):
        assert torch.equal(_forward(inp), want)                    # forcing the oracle's own decisions changes nothing
    dist = {"off": rel_l2(plain, want)}
    for name, kw in (("attn2 merged", dict(merge_cross=True)), ("another row's table", dict(roll_tables=True)), ("merged src at zero", dict(zero_merged=True))):
        with T.tome_oracle(**T.PARITY_SETTING, tables=rec, **kw):
            dist[name] = rel_l2(_forward(inp), want)
    with T.tome_oracle(**T.PARITY_SETTING, levels_shift=1):
        dist["the wrong level set"] = rel_l2(_forward(inp), want)
    print(f"hw={hw}: " + ", ".join(f"{k} {v:.3e}" for k, v in dist.items()))
    for name, d in dist.items():
        assert d >= 4 * T.PARITY_BOUND_MAX, (name, d)


def test_the_oracle_leaves_the_encoder_pass_alone_and_puts_the_module_back():
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs
    cfg, _ = _oracle_setup()
    inp = make_inputs(cfg, 2, 16, 7, 0, 96)
    orig = (OU.unet_forward, OU.transformer_2d)
    seen = []
    real = T.merge_rows

    def spy(x, slot, rows, **kw):
        seen.append(tuple(x.shape))
        return real(x, slot, rows, **kw)
    T.merge_rows = spy
    try:
        with T.tome_oracle(**T.PARITY_SETTING):
            _forward(inp)
    finally:
        T.merge_rows = real
    assert (OU.unet_forward, OU.transformer_2d) == orig
    # the main pass merges in its five level-0 blocks, attn1 only: five merges of a (2, 256, 64) map; the encoder pass (which passes
    # ``capture``) would add five more
    assert seen == [(2, 256, 64)] * 5, seen
