"""tests/branch_check.py on the CPU: the branch comparison of the VAE mid-block attention test (test_vae_ops_gpu.py) passes an
output that differs from the reference only by its bf16 rounding, and fails a 2 % error in the branch under a residual three
times the branch (rms) -- the regime the GPU test sets up.  (At 10x the bf16 rounding of out alone is ~2 % of the branch:
the two could not be told apart.)"""
import pytest
import torch

from tests.branch_check import branch_close


def _case(seed, ratio=3.0, n=512 * 4096):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(n, generator=g, dtype=torch.float64)
    x = ratio * torch.randn(n, generator=g, dtype=torch.float64)
    return x, b, g


@pytest.mark.parametrize("seed", [0, 1])
def test_branch_close_accepts_output_rounding_only(seed):
    x, b, _ = _case(seed)
    x32 = x.to(torch.bfloat16).float()       # the kernel's input is bf16
    want = (x32 + b.float())
    got = want.to(torch.bfloat16)            # exact branch, output rounded to bf16
    err, bound = branch_close(got, want, x32)
    assert err < 0.5 * bound, (err, bound)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("kind", ["scale", "noise"])
def test_branch_close_rejects_two_percent_branch_error(seed, kind):
    x, b, g = _case(seed)
    x32 = x.to(torch.bfloat16).float()
    want = x32 + b.float()
    if kind == "scale":                      # e.g. a wrong softmax scale or a dropped tail: the branch 2 % too large
        bad = b * 1.02
    else:                                    # an unstructured 2 % (rms) error in the branch
        bad = b + 0.02 * torch.randn(b.shape, generator=g, dtype=torch.float64)
    got = (x32.double() + bad).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="branch error"):
        branch_close(got, want, x32)
    # the same error is invisible to a check of the output relative to its own size: rel-L2 of out ~ 2 % / sqrt(1 + 3^2)
    rel_out = ((got.double() - want.double()).norm() / want.double().norm()).item()
    assert rel_out < 7e-3, rel_out
