"""Bit-exact tests of ``mvd_op_kid_mmd`` and ``mvd_op_fc_logits`` (csrc/kid.hip).

The MMD runs on features over {-1, 0, 1} with gamma = 1 / d a power of two and coef 1: every kernel value is (dot + d)^degree /
d^degree and every sum of them is exact in fp64 in any order (tests/test_kid_cpu.py::test_integer_inputs_are_exact), so the three
sums must equal the host's Python integers and the estimate the written fp64 expression, compared with ``torch.equal``.  The
logits run on integers in [-3, 3]: every sum is below 2^24, exact in fp32.  Without csrc/kid.hip this file fails at the
binding's symbol check."""
import pytest
import torch

import kid_ref as K

pytestmark = pytest.mark.gpu

GUARD = 4096
N_REAL, N_FAKE = 150, 141


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def index_sets(subsets, m, seed):
    """(subsets, 2, m) int32: a different permuted draw per subset and side; subset 0 repeats a row on the real side and the last
    subset one on the fake side (a repeated row is a pair like any other: the diagonal is one of positions)"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.stack([torch.randperm(N_REAL, generator=g)[:m], torch.randperm(N_FAKE, generator=g)[:m]]) for _ in range(subsets)])
    idx[0, 0, m - 1] = idx[0, 0, 0]
    idx[subsets - 1, 1, 0] = idx[subsets - 1, 1, m - 1]
    return idx.to(torch.int32)


def expected(f_real, f_fake, idx, degree):
    """sums (subsets, 3) and the estimate (subsets,) in fp64, from Python integers"""
    d, m = f_real.shape[1], idx.shape[2]
    sums, vals = [], []
    for s in range(idx.shape[0]):
        nxx, nyy, nxy = K.exact_sums(f_real[idx[s, 0].long()], f_fake[idx[s, 1].long()], degree)
        assert max(nxx, nyy, nxy) < 2 ** 53
        sxx, syy, sxy = nxx / d ** degree, nyy / d ** degree, nxy / d ** degree      # exact: d^degree is a power of two
        sums.append([sxx, syy, sxy])
        vals.append((sxx + syy) / (m * (m - 1)) - 2 * sxy / m ** 2)
    return torch.tensor(sums, dtype=torch.float64), torch.tensor(vals, dtype=torch.float64)


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("m", [2, 3, 17, 64, 65, 130])
def test_kid_mmd_integer_features(ops, m, d, degree):
    f_real, f_fake = K.integer_features(N_REAL, d, 0), K.integer_features(N_FAKE, d, 1)
    fr, ff = f_real.cuda(), f_fake.cuda()
    for subsets in (1, 3):
        idx = index_sets(subsets, m, 100 * m + subsets)
        want_sums, want = expected(f_real, f_fake, idx, degree)
        need = ops.L.lib().mvd_op_kid_workspace_bytes(subsets, m)
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        got, sums = ops.kid_mmd(fr, ff, idx.cuda(), degree, 1.0 / d, 1.0, want_sums=True, ws=ws)
        assert got.dtype == torch.float64 and got.shape == (subsets,) and sums.shape == (subsets, 3)
        assert torch.equal(sums.cpu(), want_sums), f"sums, {subsets} subset(s): {sums.cpu().tolist()} != {want_sums.tolist()}"
        assert torch.equal(got.cpu(), want), f"estimate, {subsets} subset(s): {got.cpu().tolist()} != {want.tolist()}"
        assert bool((ws[need:] == 0xA5).all()), "wrote beyond the reported workspace size"
        again, sums2 = ops.kid_mmd(fr, ff, idx.cuda(), degree, 1.0 / d, 1.0, want_sums=True)
        assert torch.equal(again, got) and torch.equal(sums2, sums)
        assert torch.equal(ops.kid_mmd(fr, ff, idx.cuda(), degree, 1.0 / d, 1.0), got)      # sums = NULL


def test_kid_mmd_rejects_bad_arguments(ops):
    from mvd_amd._lib import MvdError
    f = K.integer_features(8, 64, 0).cuda()
    idx = torch.zeros(1, 2, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(MvdError, match="m <="):
        ops.kid_mmd(f, f[:3].contiguous(), idx)
    with pytest.raises(MvdError, match="multiple of 64"):
        ops.kid_mmd(f[:, :32].contiguous(), f[:, :32].contiguous(), idx)
    with pytest.raises(MvdError, match="degree"):
        ops.kid_mmd(f, f, idx, degree=0)


@pytest.mark.parametrize("classes,d", [(1008, 2048), (16, 64)])
@pytest.mark.parametrize("n", [1, 3, 8, 17])
def test_fc_logits_small_integers(ops, n, classes, d):
    g = torch.Generator().manual_seed(n + classes)
    f = torch.randint(-3, 4, (n, d), generator=g).float()
    w = torch.randint(-3, 4, (classes, d), generator=g).float()
    want = (f.double() @ w.double().T)
    assert float(want.abs().max()) < 2 ** 24 and 9 * d < 2 ** 24
    got = ops.fc_logits(f.cuda(), w.cuda())
    assert got.dtype == torch.float32 and got.shape == (n, classes)
    assert torch.equal(got.cpu(), want.float())
    wd = w.cuda()
    for k in range(n):      # row k of the batch is the same bits as row k alone
        assert torch.equal(ops.fc_logits(f[k:k + 1].cuda(), wd)[0], got[k])


def test_fc_logits_rows_do_not_depend_on_the_batch_gaussian(ops):
    """the same on inputs whose fp32 sums DO round: any dependence of the order on n would show"""
    g = torch.Generator().manual_seed(9)
    f, w = torch.randn(17, 2048, generator=g).cuda(), torch.randn(1008, 2048, generator=g).cuda()
    full = ops.fc_logits(f, w)
    assert torch.equal(full, ops.fc_logits(f, w))
    for k in (0, 7, 8, 16):
        assert torch.equal(ops.fc_logits(f[k:k + 1].contiguous(), w)[0], full[k])
    assert torch.equal(ops.fc_logits(f[5:14].contiguous(), w), full[5:14])
    ref = f.double() @ w.double().T
    assert float((full.double() - ref).abs().max()) <= 2048 * 2.0 ** -24 * float((f.abs().double() @ w.abs().double().T).max())
