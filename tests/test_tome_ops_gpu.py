"""The token-merging operators (``ops.tome_match`` / ``tome_merge`` / ``tome_unmerge_add``, mvd_amd/csrc/tome.hip; DESIGN.md section 9
N21) on the MI355X against the fp64 definition of tests/tome_ref.py.

Scores are held to tau / 2 = 2 (C + 4) 2^-24 (``tome_ref.tau``: exact products, fp32 sums in any order, fp32 norms); decisions are
compared on the src that margin can decide (tests/test_tome_cpu.py: none is left out at the small shapes, at most 2 % at the two
large ones); merge and un-merge + add are compared bit for bit with the CPU restatement run on the GPU's own table.

Largest |score - fp64| measured on one MI355X (absolute = fraction of tau / 2):
  (1, 8, 8, 320) 1.43e-7 = 0.004;  (3, 6, 10, 320) 2.77e-7 = 0.007;  (2, 7, 9, 640) 4.77e-7 = 0.006;  (2, 16, 16, 1280) 8.87e-7 = 0.006;
  (2, 6, 6, 320) 2.18e-7 = 0.006;  (1, 64, 64, 320) 3.37e-7 = 0.009, 1 ambiguous src of 3072;  (1, 96, 96, 320) 3.31e-7 = 0.009, 7 of 6912."""
import pytest
import torch

from tests import tome_ref as T

pytestmark = pytest.mark.gpu


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops
    return ops


def _run(ops, x, H, W, r, seed=0):
    """every operator once; everything comes back on the CPU"""
    B, N, C = x.shape
    g = torch.Generator().manual_seed(1000 + seed)
    h_in = torch.randn(B, N, C, generator=g).to(torch.bfloat16)
    t_in = torch.randn(B, N - r, C, generator=g).to(torch.bfloat16)
    xg = x.cuda()
    slot, members, starts, score, best = ops.tome_match(xg, H, W, r, want_scores=True)
    slot2, members2, starts2 = ops.tome_match(xg, H, W, r)                   # (scores in the workspace: the engine's call form)
    merged = ops.tome_merge(xg, H, W, r, members, starts)
    h = h_in.cuda().clone()
    ops.tome_unmerge_add(h, t_in.cuda(), H, W, r, slot)
    torch.cuda.synchronize()
    assert torch.equal(slot, slot2) and torch.equal(members, members2) and torch.equal(starts, starts2)
    return dict(slot=slot.cpu(), members=members.cpu(), starts=starts.cpu(), score=score.cpu(), best=best.cpu(), merged=merged.cpu(),
                h_in=h_in, t_in=t_in, h_out=h.cpu())


@pytest.mark.parametrize("case", T.SMALL_CASES + T.LARGE_CASES, ids=T.case_id)
def test_decisions_and_moves_against_the_definition(case):
    (B, H, W, C, r), seed = case
    ops = _ops()
    plan = ops.tome_plan(H, W, C, r)
    dst, src = T.geometry(H, W)
    assert (plan["dst"], plan["src"], plan["rows"]) == (dst.numel(), src.numel(), H * W - r)
    assert plan["score_keys"] >= plan["src"] and plan["score_keys"] < 2 * plan["src"] and plan["member_keys"] >= H * W
    assert plan["match_workgroups"] == -(-src.numel() // 128)
    if (H, W) == (96, 96):
        assert plan["score_keys"] == 8192 and plan["member_keys"] == 16384 and H * W == plan["max_tokens"]        # the select kernel's largest form
    x = T.seeded_map(B, H, W, C, seed)
    o = _run(ops, x, H, W, r, seed)
    err, namb = T.check_decisions(x, H, W, r, o["score"], o["best"], o["slot"], o["members"], o["starts"])
    print(f"tome ops {T.case_id(case)}: score error {err:.3e} = {err / (T.tau(C) / 2):.3f} of tau / 2 ({T.tau(C) / 2:.3e}); "
          f"{namb} ambiguous src of {B * src.numel()}", flush=True)
    T.check_moves(x, o["slot"], H * W - r, o["merged"], o["h_in"], o["t_in"], o["h_out"])


@pytest.mark.parametrize("case", T.SMALL_CASES[:4], ids=T.case_id)
def test_moves_on_integer_inputs(case):
    """small integers: every sum is exact and most scores tie, whatever the table says the moves follow it bit for bit"""
    (B, H, W, C, r), seed = case
    ops = _ops()
    x = T.seeded_map(B, H, W, C, seed, integer=True)
    o = _run(ops, x, H, W, r, seed)
    slot = o["slot"].long()
    assert ((slot >= 0) & (slot < H * W - r)).all()
    T.check_moves(x, o["slot"], H * W - r, o["merged"], o["h_in"], o["t_in"], o["h_out"])


def test_planted_ties():
    """a duplicated dst row and a duplicated src row pin the two tie rules: the lower dst index, the lower token"""
    ops = _ops()
    x, r, dd, ss = T.planted_ties()
    o = _run(ops, x, 8, 8, r)
    T.check_planted_ties(x, 8, 8, r, (dd, ss), o["best"], o["slot"])
    T.check_moves(x, o["slot"], 64 - r, o["merged"], o["h_in"], o["t_in"], o["h_out"])


def test_rows_do_not_depend_on_the_batch():
    """row b of a batch of 3 equals the same row run alone, bit for bit, for all three operators (scores and tables included)"""
    ops = _ops()
    (B, H, W, C, r), seed = T.SMALL_CASES[1]
    x = T.seeded_map(B, H, W, C, seed)
    whole = _run(ops, x, H, W, r, seed)
    for b in range(B):
        xb = x[b:b + 1].cuda()
        slot, members, starts, score, best = ops.tome_match(xb, H, W, r, want_scores=True)
        merged = ops.tome_merge(xb, H, W, r, members, starts)
        h = whole["h_in"][b:b + 1].cuda().clone()
        ops.tome_unmerge_add(h, whole["t_in"][b:b + 1].cuda(), H, W, r, slot)
        for name, got in (("slot", slot), ("members", members), ("starts", starts), ("score", score), ("best", best), ("merged", merged), ("h_out", h)):
            assert torch.equal(got.cpu()[0], whole[name][b]), (b, name)


def test_refusals_come_before_any_launch():
    from mvd_amd._lib import MvdError
    ops = _ops()
    limit = ops.tome_plan(8, 8, 64, 0)["max_tokens"]
    assert limit >= 9216                                   # 96 x 96 latents must fit
    with pytest.raises(MvdError, match=str(limit)):
        ops.tome_plan(97, 96, 320, 10)
    x = torch.zeros(1, 97 * 96, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(MvdError, match=f"at most {limit}"):
        ops.tome_match(x, 97, 96, 10)
    x = torch.zeros(1, 64, 96, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(MvdError, match="multiple of 64"):
        ops.tome_match(x, 8, 8, 10)
    x = torch.zeros(1, 64, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(MvdError, match="r = -1"):
        ops.tome_match(x, 8, 8, -1)
    with pytest.raises(MvdError, match="r = 49"):
        ops.tome_match(x, 8, 8, 49)
    with pytest.raises(MvdError, match="at least 2 x 2"):
        ops.tome_match(x, 1, 64, 3)
    slot = torch.zeros(1, 64, dtype=torch.int32, device="cuda")
    with pytest.raises(MvdError, match="multiple of 64"):
        ops.tome_unmerge_add(torch.zeros(1, 64, 96, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 60, 96, dtype=torch.bfloat16, device="cuda"), 8, 8, 4, slot)
    torch.cuda.synchronize()
