"""Comparison of a residual block's BRANCH (out - x) rather than its output (test_vae_ops_gpu.py, mid-block attention).

Where a residual dominates the output, an error in the branch hides under x in any check relative to max|out| or |out|: the bf16
rounding of out alone is ~2^-9 of |out|.  ``branch_close`` measures the error against the size of the branch and allows, besides
the branch tolerance, the bf16 rounding of out -- measured on the reference itself (|| bf16(ref) - ref ||), not assumed:

    || got - ref ||  <=  tol * || ref - x ||  +  slack * || bf16(ref) - ref ||

(got - ref = (got - x) - (ref - x): the branch difference).  A kernel's own rounding of its output is a draw from the same
distribution as the reference's (same values to ~1 %, millions of elements), so slack = 1.25 leaves room for it and for
the two adding in quadrature with the branch error.  Checked on the CPU by tests/test_branch_check_cpu.py.
"""
import torch


def branch_close(got, want, x, tol=1e-2, slack=1.25, what=""):
    """got: the kernel's (bf16) output; want: the fp32 reference output; x: the residual input (same shape).
    Returns (error, bound), both relative to || want - x ||."""
    got, want, x = got.double(), want.double(), x.double()
    assert got.shape == want.shape == x.shape, (got.shape, want.shape, x.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bnorm = (want - x).norm().item()
    assert bnorm > 0, f"{what}: the reference branch is zero"
    err = (got - want).norm().item()
    rnd = (want.to(torch.bfloat16).double() - want).norm().item()
    bound = tol * bnorm + slack * rnd
    assert err <= bound, (f"{what}: branch error {err / bnorm:.4g} of ||branch|| > bound {bound / bnorm:.4g} "
                          f"(tol {tol:g} + output rounding {slack:g} x {rnd / bnorm:.4g})")
    return err / bnorm, bound / bnorm
