"""Bit-exact convolution and layout tests: the implicit-GEMM 3x3 forms (every stride / padding / upsampling mode, the fused 1x1
shortcut, row vector + residual, split-K, the blocked weight layout of the small-M kernels), the 2x2 sub-pixel upsampler, the
weight-streaming form, conv_in / conv_out and the layout / conversion kernels -- on the integer problems of exact_util.py,
compared bitwise with the fp64 reference rounded once.  One tap of one channel at a border pixel, one shortcut channel or a
wrong rounding of a tie fails these."""
import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

CONV_SHAPES = [(2, 16, 16, 64, 128), (1, 8, 12, 192, 64), (3, 6, 6, 128, 320)]          # B, H, W, cin, cout (test_ops_gpu.py)
MODES = [(1, False, False), (2, False, False), (1, True, False), (2, False, True)]      # stride, upsample, asymmetric padding
TILED_CFGS = [-1, 5, 7, 13]
SM_TILES = [0, 1, 3, 4, 5, 6]
SM_BN = {0: 64, 1: 64, 2: 128, 3: 128, 4: 160, 5: 160, 6: 320}
FUSION = (2, 8, 8, 320, 320, 128, 64)                                                  # B, H, W, cin, cout, shortcut sources
FUSION_CFGS = [-1, 2, 4, 5, 7, 10, 12, 13]
SPLIT_TILED = (2, 6, 6, 128, 320)
SPLIT_SM = (2, 6, 6, 128, 640)
UP4_SHAPES = [(1, 4, 16, 64, 320), (3, 2, 32, 128, 320), (1, 6, 8, 128, 320), (3, 8, 8, 64, 320)]
WS_SHAPES = [(2, 8, 8, 256, 64), (1, 16, 16, 128, 48), (1, 8, 32, 128, 32)]
WS_SHORTCUT = [(2, 8, 8, 128, 64, 128, 256), (1, 16, 16, 256, 32, 384, 0)]
WS_UP = [(2, 4, 8, 128, 48), (1, 8, 8, 128, 32)]
IN_OUT = [(2, 16, 12, 64), (1, 9, 10, 320)]                                             # B, H, W, C; the second width is no multiple of 4

CONV_CASES = [(c, s) for c in TILED_CFGS for s in CONV_SHAPES if c != 7 or s[4] % 320 == 0]
SM_CONV_CASES = [(t, s) for t in SM_TILES for s in CONV_SHAPES if s[4] % SM_BN[t] == 0]


def conv_shapes():
    """(B, H, W, cin, cout, sc0, sc1) of every integer 3x3 problem this file runs (for test_exact_inputs_cpu.py)"""
    return ([s + (0, 0) for s in CONV_SHAPES + [SPLIT_TILED, SPLIT_SM] + UP4_SHAPES + WS_SHAPES + WS_UP] + [FUSION, FUSION[:5] + (128, 0)]
            + WS_SHORTCUT)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def pack(w64, *more):
    """(cout, cin, 3, 3) fp64 -> the implicit-GEMM weight [cout][cin/64][ky][kx][64] (+ 1x1 shortcut columns) as fp64"""
    from mvd_amd.packing import _conv_w
    return torch.cat([_conv_w(w64).double()] + list(more), 1)


def layouts(ops, cfg, w64, run):
    """run(w, blocked): the plain packed weight; for a small-M config also packing.block_weight of it, results identical"""
    from mvd_amd.packing import block_weight
    w = X.dev(w64)
    got = run(w, None)
    if cfg >= 100:
        X.assert_same_bits(run(block_weight(w), tuple(w.shape)), got.cpu(), f"cfg {cfg}: blocked weight layout vs plain")
    return got


def run_modes(ops, cfg, shape):
    B, H, W, cin, cout = shape
    p = X.conv_problem(*shape)
    x, bias = X.dev(p.x), X.dev32(p.bias)
    for stride, ups, asym in MODES:
        want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w, stride, ups, asym), p.bias))
        got = layouts(ops, cfg, pack(p.w), lambda w, blk: ops.conv3x3(x, w, bias, stride=stride, upsample=ups, asym_pad=asym,
                                                                      force_cfg=cfg, blocked=blk))
        X.assert_same_bits(got, want, f"conv3x3 cfg {cfg} {shape} stride {stride} upsample {ups} asym {asym}")


@pytest.mark.parametrize("cfg,shape", CONV_CASES)
def test_conv3x3_modes_exact(ops, cfg, shape):
    run_modes(ops, cfg, shape)


@pytest.mark.parametrize("tile,shape", SM_CONV_CASES)
def test_sm_conv3x3_modes_exact_plain_and_blocked(ops, tile, shape):
    run_modes(ops, 100 + 10 * tile + 3, shape)


def run_fusions(ops, cfg, splitk):
    """conv2 + 1x1 shortcut over one source and over the two halves of a concatenation; conv + row vector + residual"""
    B, H, W, cin, cout, c0, c1 = FUSION
    one = X.conv_problem(B, H, W, cin, cout, c0, 0)
    two = X.conv_problem(B, H, W, cin, cout, c0, c1)
    for p, what in ((one, "one source"), (two, "two sources")):
        src = p.s0 if p.s1 is None else torch.cat([p.s0, p.s1], -1)
        want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w) + src @ p.wsc.T, p.bias))
        x, bias, s0, s1 = X.dev(p.x), X.dev32(p.bias), X.dev(p.s0), X.dev(p.s1)
        got = layouts(ops, cfg, pack(p.w, p.wsc), lambda w, blk: ops.conv3x3(x, w, bias, shortcut=s0, shortcut2=s1, force_cfg=cfg,
                                                                             splitk=splitk, blocked=blk))
        X.assert_same_bits(got, want, f"conv + shortcut over {what}, cfg {cfg} split-K {splitk}")
    p = one
    res64 = p.x * 5.0 + 1.0                                            # (cin == cout) integers in [-14, 16]: a residual of the contract's range
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w), p.bias, p.rowvec, H * W, res64))
    x, bias, rowvec, res = X.dev(p.x), X.dev32(p.bias), X.dev32(p.rowvec), X.dev(res64)
    got = layouts(ops, cfg, pack(p.w), lambda w, blk: ops.conv3x3(x, w, bias, rowvec=rowvec, res=res, force_cfg=cfg, splitk=splitk,
                                                                  blocked=blk))
    X.assert_same_bits(got, want, f"conv + row vector + residual, cfg {cfg} split-K {splitk}")


@pytest.mark.parametrize("cfg", FUSION_CFGS)
def test_conv3x3_resnet_fusions_exact(ops, cfg):
    run_fusions(ops, cfg, 1)


@pytest.mark.parametrize("splitk", [1, 4])
@pytest.mark.parametrize("tile", [t for t in SM_TILES if FUSION[4] % SM_BN[t] == 0])
def test_sm_conv3x3_resnet_fusions_exact(ops, tile, splitk):
    run_fusions(ops, 100 + 10 * tile + 4, splitk)


@pytest.mark.parametrize("splitk", [2, 3, 5])
@pytest.mark.parametrize("cfg", [-1, 7, 10, 13, 104, 114, 134, 154, 164])
def test_conv3x3_splitk_exact(ops, cfg, splitk):
    shape = SPLIT_SM if cfg >= 100 else SPLIT_TILED
    p = X.conv_problem(*shape)
    x, bias = X.dev(p.x), X.dev32(p.bias)
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w), p.bias))
    got = layouts(ops, cfg, pack(p.w), lambda w, blk: ops.conv3x3(x, w, bias, force_cfg=cfg, splitk=splitk, blocked=blk))
    X.assert_same_bits(got, want, f"conv3x3 cfg {cfg} split-K {splitk}")


# ------------------------------------------------------------------------------------------------ 2x2 sub-pixel upsampler
@pytest.mark.parametrize("shape", UP4_SHAPES)
def test_conv3x3_up4_exact(ops, shape):
    """pack_up4 sums at most four ternary taps -- exact in bf16 -- so the four 2x2 convolutions equal the nine-tap reference bitwise"""
    from mvd_amd.packing import pack_up4
    p = X.conv_problem(*shape)
    w4 = pack_up4(X.f32(p.w))
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w, upsample=True), p.bias))
    got = ops.conv3x3_up4(X.dev(p.x), w4.cuda(), X.dev32(p.bias))
    X.assert_same_bits(got, want, f"conv3x3_up4 {shape}")


# ------------------------------------------------------------------------------------------------ weight-streaming form
def ws_variants(h, w):
    return [0, 1] + ([2] if w == 16 and (h * w) % 128 == 0 else [])


@pytest.mark.parametrize("shape", WS_SHAPES)
def test_conv_ws_dense_exact(ops, shape):
    from mvd_amd.packing import pack_ws
    B, H, W, c, n = shape
    p = X.conv_problem(*shape)
    res64 = X.gemm_problem(B * H * W, n, 64).res.reshape(B, H, W, n)
    wp, x, bias = pack_ws(X.f32(p.w)).cuda(), X.dev(p.x), X.dev32(p.bias)
    acc = X.conv_acc(p.x, p.w)
    for v in ws_variants(H, W):
        X.assert_same_bits(ops.conv3x3_ws(x, wp, bias, n, variant=v), X.round_once(X.epilogue(acc, p.bias)), f"ws {shape} variant {v}")
        got = ops.conv3x3_ws(x, wp, bias, n, rowvec=X.dev32(p.rowvec), res=X.dev(res64), variant=v)
        X.assert_same_bits(got, X.round_once(X.epilogue(acc, p.bias, p.rowvec, H * W, res64)), f"ws {shape} variant {v} row vector + residual")


@pytest.mark.parametrize("shape", WS_SHORTCUT)
def test_conv_ws_shortcut_exact(ops, shape):
    from mvd_amd.packing import pack_ws
    B, H, W, c, n, s0, s1 = shape
    p = X.conv_problem(*shape)
    src = p.s0 if p.s1 is None else torch.cat([p.s0, p.s1], -1)
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w) + src @ p.wsc.T, p.bias))
    wp = pack_ws(X.f32(p.w), X.f32(p.wsc)).cuda()
    for v in ws_variants(H, W):
        got = ops.conv3x3_ws(X.dev(p.x), wp, X.dev32(p.bias), n, shortcut=X.dev(p.s0), shortcut2=X.dev(p.s1), variant=v)
        X.assert_same_bits(got, want, f"ws + shortcut {shape} variant {v}")


@pytest.mark.parametrize("shape", WS_UP)
def test_conv_ws_upsample_exact(ops, shape):
    from mvd_amd.packing import pack_ws
    B, H, W, c, n = shape
    p = X.conv_problem(*shape)
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w, upsample=True), p.bias))
    wp = pack_ws(X.f32(p.w)).cuda()
    for v in ws_variants(2 * H, 2 * W):
        got = ops.conv3x3_ws(X.dev(p.x), wp, X.dev32(p.bias), n, variant=v, upsample=True)
        X.assert_same_bits(got, want, f"ws upsample {shape} variant {v}")


# ------------------------------------------------------------------------------------------------ conv_in / conv_out
@pytest.mark.parametrize("B,H,W,c", IN_OUT)
def test_conv_in_out_exact(ops, B, H, W, c):
    from mvd_amd.packing import _conv_w
    p = X.conv_problem(B, H, W, 4, c)                     # conv_in: 4 -> c channels, fp32 weight (cout, 3, 3, cin)
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w), p.bias))
    got = ops.conv_in(X.dev(p.x), X.dev32(p.w.permute(0, 2, 3, 1)), X.dev32(p.bias))
    X.assert_same_bits(got, want, "conv_in")
    p = X.conv_problem(B, H, W, c, 4, seed=1)             # conv_out: c -> 4 channels, NCHW fp32 output: no rounding at all
    want = X.round_once(X.epilogue(X.conv_acc(p.x, p.w), p.bias), out_f32=True).permute(0, 3, 1, 2).contiguous()
    got = ops.conv_out(X.dev(p.x), X.dev(_conv_w(p.w, tap_major=True).double()), X.dev32(p.bias))
    X.assert_same_bits(got, want, "conv_out")


# ------------------------------------------------------------------------------------------------ layout and conversion
def test_layout_round_trip_and_film_exact(ops):
    g = torch.Generator().manual_seed(11)
    B, c, H, W = 3, 5, 7, 9                               # ragged: no dimension is a multiple of anything
    x = torch.randint(-255, 256, (B, c, H, W), generator=g).double()
    nhwc = ops.nchw_to_nhwc(X.dev32(x))
    X.assert_same_bits(nhwc, X.bf(x.permute(0, 2, 3, 1).contiguous()), "nchw_to_nhwc")
    X.assert_same_bits(ops.nhwc_to_nchw(nhwc), X.f32(x), "nhwc_to_nchw(nchw_to_nhwc(x))")
    # FiLM with power-of-two scales: x * s is exact, + shift is exact in fp32, one rounding (odd sums above 256 are ties)
    s = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], dtype=torch.float64)[torch.randint(0, 5, (B, c), generator=g)]
    s = s * (torch.randint(0, 2, (B, c), generator=g).double() * 2 - 1)
    t = torch.randint(-8, 9, (B, c), generator=g).double()
    want = X.round_once((x * s[:, :, None, None] + t[:, :, None, None]).permute(0, 2, 3, 1).contiguous())
    X.assert_same_bits(ops.nchw_to_nhwc(X.dev32(x), X.dev32(s), X.dev32(t)), want, "nchw_to_nhwc + FiLM")
    B, hw, c = 3, 35, 24
    x = torch.randint(-255, 256, (B, hw, c), generator=g).double()
    s = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], dtype=torch.float64)[torch.randint(0, 5, (B, c), generator=g)]
    t = torch.randint(-8, 9, (B, c), generator=g).double()
    X.assert_same_bits(ops.film(X.dev(x), X.dev32(s), X.dev32(t)), X.round_once(x * s[:, None] + t[:, None]), "film")


def f32_table():
    """fp32 bit patterns around every rounding decision of fp32 -> bf16 (no subnormals: nothing in the project defines them)"""
    his = [0x3F80, 0x3F81, 0x3FFF, 0x4000, 0x4049, 0x42C8, 0x0080, 0x0081, 0x7F7E, 0x7F7F, 0x7F00, 0x0100]
    los = [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]    # exact, just above, one ulp below a tie, the tie (hi even / odd), one above
    pats = [(h << 16) | lo for h in his for lo in los]
    pats += [p | 0x80000000 for p in pats]
    pats += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000,   # +-0, +-inf
             0x7F7F7FFF, 0x7F7F8000, 0xFF7F7FFF, 0xFF7F8000,   # the largest value that stays finite, the first that rounds to inf
             0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]   # NaNs
    t = torch.tensor(pats, dtype=torch.int64)
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


@pytest.mark.parametrize("n", [1000, 4096 * 256 + 333])      # not a multiple of the 256-thread block; beyond the 4096-block grid cap
def test_f32_to_bf16_exact(ops, n):
    table = f32_table()
    g = torch.Generator().manual_seed(n)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    expo = (bits >> 23) & 0xFF
    bits = torch.where(expo == 0, bits | (1 << 23), bits)      # subnormal / zero patterns -> normal ones
    bits[:table.numel()] = table
    bits[-table.numel():] = table
    x = bits.view(torch.float32)
    want = x.to(torch.bfloat16)
    got = ops.f32_to_bf16(x.cuda()).cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN must stay NaN (and nothing else may become one)"
    X.assert_same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), f"f32_to_bf16 n={n}")
