"""Bit-exact tests of the ReLU epilogue of the lock-step GEMM / implicit 3x3 convolution (gemm_relu.hip) and of the 2x2 max-pool
(vgg.hip), on the integer problems of exact_util.py.

The bias of a problem is replaced by minus the rounded per-channel median of the accumulator, so that about half of the pre-ReLU
outputs are negative and half positive (asserted: >= 40 % each): a ReLU that is missing, applied to the wrong operand or applied
after the rounding cannot pass.  Everything is an integer far below 2^24, so the reference -- fp64 on the CPU, max(., 0), ONE
rounding -- is exact and the comparison is ``torch.equal`` on the bit patterns.  Every lock-step tile config that takes the N
(3 / 4 / 5 register-staged, 11 / 12 / 13 LDS-DMA, and the heuristic), unsplit and through the split-K reduce pass, bf16 and fp32
outputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_util as X

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 8, 64, 64), (1, 6, 10, 128, 128), (1, 4, 4, 512, 512), (1, 5, 7, 64, 128)]      # B, H, W, cin, cout
TILE_BN = {3: 128, 4: 64, 5: 64}                                                              # tile config -> columns per tile
DENSE = (200, 128, 192)                                                                       # m, n, k: m is no multiple of a tile
POOL_SHAPES = [(2, 8, 8, 64), (1, 5, 7, 512), (1, 2, 2, 128)]


def configs(n):
    """every lock-step tile config that takes N = n with a ReLU: -1 (heuristic), register staging, LDS-DMA staging (+8)"""
    tiles = [c for c, bn in TILE_BN.items() if n % bn == 0]
    return [-1] + tiles + [c + 8 for c in tiles]


CASES = [(s, c) for s in SHAPES for c in configs(s[4])]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def centred_bias(acc):
    """minus the rounded per-channel median: an integer (checked with X.f32 by the callers)"""
    return -acc.reshape(-1, acc.shape[-1]).median(0).values.round()


def balanced(pre, what):
    neg, pos = float((pre < 0).double().mean()), float((pre > 0).double().mean())
    assert neg >= 0.4 and pos >= 0.4, f"{what}: {neg:.1%} negative, {pos:.1%} positive pre-ReLU outputs"


@functools.lru_cache(maxsize=8)
def conv_case(shape):
    """(problem, bias fp64, pre-ReLU output fp64) of one shape, computed once for all its configs"""
    p = X.conv_problem(*shape)
    acc = X.conv_acc(p.x, p.w)
    bias = centred_bias(acc)
    X.f32(bias)
    pre = X.epilogue(acc, bias)
    balanced(pre, f"conv {shape}")
    return p, bias, pre


def pack(w64):
    from mvd_amd.packing import _conv_w
    return X.dev(_conv_w(w64).double())


@pytest.mark.parametrize("shape,cfg", CASES)
def test_conv3x3_relu_exact(ops, shape, cfg):
    p, bias, pre = conv_case(shape)
    x, w, b = X.dev(p.x), pack(p.w), X.dev32(bias)
    for splitk in (1, 4):
        for out_f32 in (False, True):
            got = ops.conv3x3_relu(x, w, b, relu=True, out_f32=out_f32, force_cfg=cfg, splitk=splitk)
            X.assert_same_bits(got, X.round_once(pre.clamp(min=0.0), out_f32), f"conv3x3_relu {shape} cfg {cfg} split-K {splitk} fp32 {out_f32}")
    if cfg < 0:
        assert ops.last_gemm_plan()["cfg"] in (3, 4, 5)
        # relu = 0 through the same entry point: the plain kernels, negative outputs kept
        got = ops.conv3x3_relu(x, w, b, relu=False, out_f32=True)
        X.assert_same_bits(got, X.round_once(pre, True), f"conv3x3_relu(relu=False) {shape}")


@pytest.mark.parametrize("cfg", configs(DENSE[1]))
def test_linear_relu_exact(ops, cfg):
    m, n, k = DENSE
    p = X.gemm_problem(m, n, k)
    acc = X.gemm_acc(m, n, k)
    bias = centred_bias(acc)
    X.f32(bias)
    pre = X.epilogue(acc, bias)
    balanced(pre, f"dense {DENSE}")
    for splitk in (1, 3):
        for out_f32 in (False, True):
            got = ops.linear_relu(X.dev(p.a), X.dev(p.w), X.dev32(bias), relu=True, out_f32=out_f32, force_cfg=cfg, splitk=splitk)
            X.assert_same_bits(got, X.round_once(pre.clamp(min=0.0), out_f32), f"linear_relu cfg {cfg} split-K {splitk} fp32 {out_f32}")


def test_relu_is_refused_where_no_kernel_has_it(ops):
    """tiles without a ReLU form (128x160, 256x320) and the small-M kernels are errors, never a launch that drops the ReLU"""
    from mvd_amd._lib import MvdError
    p = X.conv_problem(1, 4, 4, 64, 320)                  # N = 320: every tile family takes the plain problem (test_exact_conv_gpu.py)
    x, w, b = X.dev(p.x), pack(p.w), X.dev32(p.bias)
    for cfg in (2, 7, 10, 103):
        with pytest.raises(MvdError):
            ops.conv3x3_relu(x, w, b, relu=True, force_cfg=cfg)
    # the heuristic never leaves the tiles that have the ReLU: N = 320 goes to the 128x64 tile
    pre = X.epilogue(X.conv_acc(p.x, p.w), p.bias)
    X.assert_same_bits(ops.conv3x3_relu(x, w, b, relu=True), X.round_once(pre.clamp(min=0.0)), "conv3x3_relu N = 320")
    assert ops.last_gemm_plan()["cfg"] == 4


@pytest.mark.parametrize("B,H,W,c", POOL_SHAPES)
def test_maxpool2x2_exact(ops, B, H, W, c):
    g = torch.Generator().manual_seed(B + 3 * H + 5 * W + c)
    x = (torch.randn(B, H, W, c, generator=g) * 4).to(torch.bfloat16)
    x[0, 0, 0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 2.0 ** -126, 0.5]).to(torch.bfloat16)
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    assert want.shape == (B, H // 2, W // 2, c)
    # the output sits in a larger buffer of a sentinel value: nothing beyond the B x H/2 x W/2 x c outputs may be written
    n, guard = want.numel(), 4096
    buf = torch.full((n + guard,), -7.0, dtype=torch.bfloat16, device="cuda")
    ops.maxpool2x2(x.cuda(), out=buf)
    X.assert_same_bits(buf[:n].reshape(want.shape), want, f"maxpool2x2 {(B, H, W, c)}")
    assert torch.equal(buf[n:].cpu(), torch.full((guard,), -7.0, dtype=torch.bfloat16)), "maxpool2x2 wrote beyond its output"
    X.assert_same_bits(ops.maxpool2x2(x.cuda()), want, "maxpool2x2 (own buffer)")
