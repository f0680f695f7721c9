"""``ops.todo_downsample`` (``mvd_op_todo_downsample``) on the MI355X, bit for bit against the CPU
restatement of tests/todo_ref.py: both methods, fused rows of stride 3C and 4C, Gaussian, integer and order-sensitive ("cancel")
inputs, K and V each against their own columns.  tests/test_todo_cpu.py shows that every op-level fault -- the wrong corner, a cell
off by one column, an incomplete last cell included, the sum reversed, truncation, V from K's columns, the batch stride of the
compact rows -- fails these checks.  Composition with ``ops.attention`` (nq = H W queries against nk = Nk pooled keys) is held to
the project's operator tolerance: max|err| at most one bf16 ulp of the largest output (2^-7 max|ref|) against fp64 attention on
the reference-pooled K/V."""
import ctypes as C

import pytest
import torch

from tests import todo_ref as T

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def inputs():
    """the fused rows of every (case, width, kind), made once and left unchanged"""
    _need_gpu()
    return {(c, w, k): T.fused_rows(c, w, k) for c in T.OP_CASES for w in T.OP_WIDTHS for k in T.OP_INPUTS}


def _kv(dev, C_):
    return dev[..., C_:2 * C_], dev[..., 2 * C_:3 * C_]


@pytest.mark.parametrize("width", T.OP_WIDTHS, ids=["ld3C", "ld4C"])
@pytest.mark.parametrize("case", T.OP_CASES, ids=T.case_id)
def test_downsample_is_the_restatement_bit_for_bit(inputs, case, width):
    from mvd_amd import ops
    B, H, W, C_, f = case
    for kind in T.OP_INPUTS:
        qkv = inputs[(case, width, kind)]
        dev = qkv.cuda()
        for method in T.METHODS:
            out = ops.todo_downsample(*_kv(dev, C_), H, W, f, method)
            T.check_op(out.cpu(), qkv, case, method)
            if width == 3:                                       # the fused buffer itself, v=None: the same launch
                assert torch.equal(ops.todo_downsample(dev, None, H, W, f, method), out)
            else:
                assert torch.equal(ops.todo_downsample(dev, None, H, W, f, method, channels=C_), out)


@pytest.mark.parametrize("case", [(3, 6, 10, 320, 2), (2, 7, 10, 320, 3)], ids=T.case_id)
def test_nothing_outside_the_output_is_written_and_a_row_does_not_depend_on_the_batch(inputs, case):
    from mvd_amd import ops
    B, H, W, C_, f = case
    Nk = T.key_grid(H, W, f)[2]
    qkv = inputs[(case, 4, "gauss")]
    dev = qkv.cuda()
    n = B * Nk * 2 * C_
    for method in T.METHODS:
        guard = torch.full((n + 2 * 4096,), -7.0, dtype=torch.bfloat16, device="cuda")
        out = guard[4096:4096 + n].view(B, Nk, 2 * C_)
        ops.todo_downsample(*_kv(dev, C_), H, W, f, method, out=out)
        assert (guard[:4096] == -7.0).all() and (guard[4096 + n:] == -7.0).all()
        T.check_op(out.cpu(), qkv, case, method)
        for b in range(B):                                       # row b of the batch == that image alone (another grid)
            alone = dev[b:b + 1].clone()
            assert torch.equal(ops.todo_downsample(*_kv(alone, C_), H, W, f, method), out[b:b + 1])


def test_every_refusal_comes_before_a_launch_and_leaves_the_output_alone():
    _need_gpu()
    from mvd_amd import _lib as L
    from mvd_amd import ops
    B, H, W, C_, f = 2, 8, 8, 64, 2
    qkv = torch.randn(B, H * W, 3 * C_, device="cuda").to(torch.bfloat16)
    pad = torch.zeros(B * H * W * 3 * C_ + 64, dtype=torch.bfloat16, device="cuda")
    Nk = 16
    out = torch.full((B, Nk, 2 * C_), -7.0, dtype=torch.bfloat16, device="cuda")
    k, v = qkv.data_ptr() + 2 * C_, qkv.data_ptr() + 4 * C_
    ok = dict(k=k, v=v, ld=3 * C_, B=B, H=H, W=W, C=C_, f=f, method=0, out=out.data_ptr())
    lib = L.lib()

    def call(**change):
        a = {**ok, **change}
        p = [C.c_void_p(a[n]) if a[n] else None for n in ("k", "v")]
        return lib.mvd_op_todo_downsample(p[0], p[1], a["ld"], a["B"], a["H"], a["W"], a["C"], a["f"], a["method"],
                                          C.c_void_p(a["out"]) if a["out"] else None, L.stream())
    refusals = [(dict(f=1), "factor"), (dict(f=5), "factor"), (dict(f=0), "factor"), (dict(method=2), "method"), (dict(method=-1), "method"),
                (dict(C=60), "multiple of 8"), (dict(ld=3 * C_ + 4), "row stride"), (dict(ld=C_ - 8), "row stride"), (dict(k=0), "null"), (dict(v=0), "null"),
                (dict(out=0), "null"), (dict(k=k + 2), "aligned"), (dict(v=v + 8), "aligned"), (dict(out=out.data_ptr() + 2), "aligned"),
                (dict(H=1), "no complete"), (dict(W=1), "no complete"), (dict(f=4, H=3), "no complete"),
                (dict(out=qkv.data_ptr()), "overlaps"), (dict(out=qkv.data_ptr() + qkv.numel() * 2 - 64), "overlaps"),
                (dict(k=pad.data_ptr() + 128, v=pad.data_ptr() + 256, out=pad.data_ptr()), "overlaps")]
    for change, msg in refusals:
        assert call(**change) == -1, change
        assert msg in L.last_error(), (change, L.last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (pad == 0).all()
    assert call() == 0
    T.check_op(out.cpu(), qkv.cpu(), (B, H, W, C_, f), "nearest")
    # the Python wrapper's own words
    with pytest.raises(L.MvdError, match="method must be one of"):
        ops.todo_downsample(*_kv(qkv, C_), H, W, f, "bilinear")
    with pytest.raises(L.MvdError, match="share a row stride"):
        ops.todo_downsample(qkv[..., C_:2 * C_], qkv[..., 2 * C_:3 * C_].contiguous(), H, W, f, "area")
    with pytest.raises(L.MvdError, match="expected out"):
        ops.todo_downsample(*_kv(qkv, C_), H, W, f, "area", out=out[:, :8])
    with pytest.raises(L.MvdError, match="factor"):
        ops.todo_downsample(*_kv(qkv, C_), H, W, 1, "area")


@pytest.mark.parametrize("case", [(1, 8, 8, 320, 2), (2, 7, 9, 640, 2)], ids=T.case_id)
@pytest.mark.parametrize("method", T.METHODS)
def test_attention_on_the_pooled_keys(case, method):
    """every query of the map against the Nk pooled keys: the launch the engine makes (ldk = ldv = 2C, K | V in one compact buffer)"""
    _need_gpu()
    from mvd_amd import ops
    B, H, W, C_, f = case
    heads = C_ // 64
    g = torch.Generator().manual_seed(H * W + C_)
    qkv = torch.randn(B, H * W, 3 * C_, generator=g).to(torch.bfloat16)
    dev = qkv.cuda()
    kv = ops.todo_downsample(*_kv(dev, C_), H, W, f, method)
    T.check_op(kv.cpu(), qkv, case, method)
    Nk = kv.shape[1]
    got = ops.attention(dev[..., :C_], kv[..., :C_], kv[..., C_:], heads).cpu().double()
    ref = T.reference_kv(qkv, C_, H, W, f, method).double()

    def split(t, n):
        return t.reshape(B, n, heads, 64).transpose(1, 2)
    want = torch.nn.functional.scaled_dot_product_attention(split(qkv[..., :C_].double(), H * W), split(ref[..., :C_], Nk), split(ref[..., C_:], Nk))
    want = want.transpose(1, 2).reshape(B, H * W, C_)
    err, ulp = (got - want).abs().max().item(), 2.0 ** -7 * want.abs().max().item()
    print(f"attention on pooled keys {case} {method}: nq {H * W} nk {Nk}: max|err| {err:.4g}, one bf16 ulp of the largest output {ulp:.4g}")
    assert err <= ulp
