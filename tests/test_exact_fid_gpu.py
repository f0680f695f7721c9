"""Bit-exact tests of the kernels FID adds (csrc/fid.hip): the implicit-GEMM convolution with its slice epilogue, the three 3x3
pools, the TF1-legacy resize front end, the global mean and the fp64 feature statistics.

Convolutions, the mean and the statistics run on small integers (tests/exact_util.py's generators): every product and partial sum
is far below 2^24 (2^53 for the statistics), so the fp64 reference on the CPU is exact in any order and the comparison is
``torch.equal`` on the bit patterns, ONE rounding to bf16 at the end.  The pools and the front end are compared with restatements
that perform the same fp32 operations in the same order.  Inputs are read from a channel slice of a wider buffer whose other
channels hold NaN; outputs go into a slice of a wider buffer of a sentinel value, followed by a guard: nothing outside the slice
may change.  Without csrc/fid.hip this file fails at the binding's symbol check."""
import pytest
import torch
import torch.nn.functional as F

import exact_util as X
import fid_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def sliced_input(x64, ld, off):
    """(B, H, W, c) fp64 bf16 values -> a (B, H, W, ld) bf16 device buffer with x in channels [off, off + c) and NaN elsewhere"""
    B, H, W, c = x64.shape
    buf = torch.full((B, H, W, ld), float("nan"), dtype=torch.bfloat16)
    buf[..., off:off + c] = X.bf(x64)
    return buf.cuda()


def sentinel_output(shape, dtype):
    """a flat device buffer of shape + GUARD sentinel elements and its view of ``shape``"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def check_slice(flat, view, c_off, c, want, what):
    """channels [c_off, c_off + c) of ``view`` equal ``want`` bit for bit; every other element of the buffer is the sentinel"""
    got = view.cpu()
    X.assert_same_bits(got[..., c_off:c_off + c].contiguous(), want, what)
    rest = torch.cat([got[..., :c_off].reshape(-1), got[..., c_off + c:].reshape(-1), flat[view.numel():].cpu()])
    assert torch.equal(rest, torch.full_like(rest, SENTINEL)), f"{what}: wrote outside its slice"


# ------------------------------------------------------------------------------------------------ convolution
# (kh, kw, stride, pad_h, pad_w): every form of packing.INCEPTION_FID_LAYERS (asserted below)
FORMS = ((1, 1, 1, 0, 0), (3, 3, 2, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (5, 5, 1, 2, 2), (1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1),
         (3, 1, 1, 1, 0))
# (form, B, H, W, cin, cout): every form; maps of 5 x 7, 9 x 9 and 8 x 8; batch 1 and 3; cin and cout in {32, 48, 80, 288 / 320};
# M = 35, 105, 243 (not multiples of the 64-row tile, several workgroups) and 64; cout 80 and 320: a partly filled last 64-column tile
CASES = (
    (FORMS[0], 1, 5, 7, 48, 80), (FORMS[0], 3, 9, 9, 288, 320), (FORMS[1], 3, 9, 9, 32, 48), (FORMS[1], 1, 8, 8, 288, 32),
    (FORMS[2], 1, 5, 7, 80, 32), (FORMS[2], 3, 8, 8, 32, 80), (FORMS[3], 3, 5, 7, 48, 48), (FORMS[3], 1, 9, 9, 80, 320),
    (FORMS[4], 1, 9, 9, 48, 80), (FORMS[4], 3, 5, 7, 32, 32), (FORMS[5], 1, 8, 8, 80, 48), (FORMS[5], 3, 5, 7, 32, 320),
    (FORMS[6], 3, 9, 9, 48, 32), (FORMS[6], 1, 5, 7, 288, 80), (FORMS[7], 1, 8, 8, 32, 80), (FORMS[7], 3, 9, 9, 80, 48),
    (FORMS[8], 1, 5, 7, 48, 320), (FORMS[8], 3, 8, 8, 288, 32),
    (FORMS[6], 1, 9, 9, 768, 48),      # K = 7 x 1 x 768 = 5376: 168 K steps, taps that cross the image border and the row tile
)


def test_forms_are_the_networks():
    from mvd_amd.packing import INCEPTION_FID_CONVS
    assert {(e[7], e[8], e[9], e[10], e[11]) for e in INCEPTION_FID_CONVS} == set(FORMS)


def conv_problem(form, B, H, W, cin, cout):
    """integers in [-3, 3] against ternary weights, tilted along the channels so that outputs reach the binades with bf16 ties;
    the bias centres the pre-ReLU outputs so that about half are negative"""
    kh, kw, stride, ph, pw = form
    g = X._gen(B + 3 * H + 5 * W + 7 * cin + 11 * cout + 13 * kh + 17 * kw + 19 * stride)
    s = X._sign(g, cin)
    x = X._tilted(g, B * H * W, cin, -3, 3, s).reshape(B, H, W, cin)
    w = X._tilted(g, cout * kh * kw, cin, -1, 1, s).reshape(cout, kh, kw, cin).permute(0, 3, 1, 2).contiguous()
    acc = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1).contiguous()
    bias = -acc.reshape(-1, cout).median(0).values.round() + X._ints(g, (cout,), -2, 2)
    return x, w, bias, acc + bias


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"k{c[0][0]}x{c[0][1]}s{c[0][2]}-b{c[1]}-{c[2]}x{c[3]}-{c[4]}to{c[5]}")
def test_conv_relu_slice_exact(ops, case, out_f32):
    from mvd_amd.packing import fid_cin_pad, pack_slice_conv
    form, B, H, W, cin, cout = case
    kh, kw, stride, ph, pw = form
    x, w, bias, pre = conv_problem(form, B, H, W, cin, cout)
    assert 3 * kh * kw * cin + 16 < 2 ** 24
    neg = float((pre < 0).double().mean())
    assert 0.25 <= neg <= 0.75, f"{neg:.1%} of the pre-ReLU outputs are negative"
    wp = pack_slice_conv(w)
    pad = fid_cin_pad(cin)
    assert wp.shape == (cout, kh * kw * pad)
    if pad != cin:      # the padded K columns are zeros
        assert torch.count_nonzero(wp.reshape(cout, kh * kw, pad)[:, :, cin:]) == 0
    cin_off, c_off = 16, 32
    xin = sliced_input(x, cin + 48, cin_off)
    oh, ow = pre.shape[1:3]
    flat, view = sentinel_output((B, oh, ow, cout + 48), torch.float32 if out_f32 else torch.bfloat16)
    ops.conv_relu_slice(xin, X.dev(wp), X.dev32(bias), kh, kw, stride, (ph, pw), cin_off=cin_off, cin=cin, out=view, c_off=c_off, out_f32=out_f32)
    check_slice(flat, view, c_off, cout, X.round_once(pre.clamp(min=0.0), out_f32), f"conv_relu_slice {case} fp32 {out_f32}")


def test_conv_relu_slice_own_buffer_and_whole_rows(ops):
    """no slices on either side (ld = c, offsets 0) and the output allocated by the binding"""
    from mvd_amd.packing import pack_slice_conv
    form = FORMS[3]
    x, w, bias, pre = conv_problem(form, 2, 9, 9, 32, 48)
    got = ops.conv_relu_slice(X.dev(x), X.dev(pack_slice_conv(w)), X.dev32(bias), 3, 3, 1, (1, 1))
    X.assert_same_bits(got, X.round_once(pre.clamp(min=0.0)), "conv_relu_slice, whole rows")


def test_conv_relu_slice_rejects_what_it_cannot_run(ops):
    from mvd_amd._lib import MvdError
    from mvd_amd.packing import pack_slice_conv
    x, w, bias, _ = conv_problem(FORMS[0], 1, 5, 7, 48, 80)
    wp, b = X.dev(pack_slice_conv(w)), X.dev32(bias)
    with pytest.raises(MvdError, match="multiples of 16"):
        ops.conv_relu_slice(X.dev(x), wp, b, 1, 1, cin_off=8, cin=40)
    with pytest.raises(MvdError, match="1x1, 3x3"):
        ops.conv_relu_slice(X.dev(x), wp, b, 1, 1, stride=3)


# ------------------------------------------------------------------------------------------------ pools
def pool_reference(x, mode):
    """x (B, H, W, c) bf16 -> bf16: "avg" as the kernel writes it -- the fp32 sum of the in-image taps in (ky, kx) order, a true
    division by their count (4 / 6 / 9 at corners / edges / inside), one rounding; the maxima through F.max_pool2d"""
    xf = x.float().permute(0, 3, 1, 2)
    if mode != "avg":
        y = F.max_pool2d(xf, 3, 1, 1) if mode == "max1" else F.max_pool2d(xf, 3, 2)
        return y.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    B, c, H, W = xf.shape
    xp, ones = F.pad(xf, (1, 1, 1, 1)), F.pad(torch.ones(1, 1, H, W), (1, 1, 1, 1))
    s, n = torch.zeros_like(xf), torch.zeros(1, 1, H, W)
    for ky in range(3):
        for kx in range(3):
            s = s + xp[:, :, ky:ky + H, kx:kx + W]
            n = n + ones[:, :, ky:ky + H, kx:kx + W]
    assert n[0, 0, 0, 0] == 4 and n[0, 0, 0, 1] == 6 and n[0, 0, 1, 1] == 9
    return (s / n).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (2, 8, 8)])
@pytest.mark.parametrize("mode", ["avg", "max1", "max2"])
def test_pool3x3_slice_exact(ops, mode, B, H, W):
    c = 48
    g = torch.Generator().manual_seed(B + 3 * H + 5 * W)
    x = (torch.randn(B, H, W, c, generator=g) * 4).to(torch.bfloat16)
    x[0, 0, 0, :8] = torch.tensor([0.0, 0.25, 1.0, -1.0, 3.0e38, -3.0e38, 2.0 ** -120, 0.5]).to(torch.bfloat16)
    if mode != "avg":
        x[0, 1, 1] = -3.0e38      # a window of very negative values: the (zero or absent) padding must not win
        x[0, 0, 1] = -3.0e38
        x[0, 1, 0] = -3.0e38
        x[0, 0, 0, 8:] = -3.0e38
    want = pool_reference(x, mode)
    assert torch.isfinite(want.float()).all()
    cin_off, c_off = 16, 32
    xin = sliced_input(x.double(), c + 32, cin_off)
    flat, view = sentinel_output(tuple(want.shape[:3]) + (c + 64,), torch.bfloat16)
    ops.pool3x3_slice(xin, mode, cin_off=cin_off, c=c, out=view, c_off=c_off)
    check_slice(flat, view, c_off, c, want, f"pool3x3_slice {mode} {(B, H, W)}")
    X.assert_same_bits(ops.pool3x3_slice(x.cuda(), mode), want, f"pool3x3_slice {mode} (own buffer)")


# ------------------------------------------------------------------------------------------------ front end
def front_end_inputs(kind, B, H, W):
    g = torch.Generator().manual_seed(B + 3 * H + 5 * W)
    k = torch.randint(0, 256, (B, 3, H, W), generator=g)
    k[0, :, 0, :4] = torch.tensor([0, 255, 1, 254]).view(1, 4)
    if kind == "uint8":
        return k.to(torch.uint8)
    # k / 255 and a step of 2^-20 to either side: x * 255 lands on, just above and just below an integer (the truncation),
    # and below 0 / above 1 at the ends (the clamp)
    step = torch.randint(-1, 2, (B, 3, H, W), generator=g).float() * 2.0 ** -20
    return k.float() / 255.0 + step


@pytest.mark.parametrize("kind", ["uint8", "fp32"])
@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (1, 40, 56), (1, 299, 299), (1, 512, 384)], ids=["up", "anisotropic", "identity", "down"])
def test_resize_tf1_exact(ops, kind, B, H, W):
    x = front_end_inputs(kind, B, H, W)
    want = R.front_end(x).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    if kind == "fp32":
        q = R.quantise(x)
        assert q.min() == 0 and q.max() == 255 and (x.min() < 0 or x.max() > 1)
        assert float((q != torch.round(x * 255.0)).float().mean()) > 0.1, "no input sits just below an integer"
    if (H, W) == (299, 299):      # the identity: the quantised image itself, normalised
        src = x.float() if kind == "uint8" else R.quantise(x)
        assert torch.equal(want.float(), ((src - 128.0) / 128.0).permute(0, 2, 3, 1).to(torch.bfloat16).float())
    got = ops.resize_tf1(x.cuda()).cpu()
    assert got.shape == (B, 299, 299, 16)
    X.assert_same_bits(got[..., :3].contiguous(), want, f"resize_tf1 {kind} {(B, H, W)}")
    assert torch.count_nonzero(got[..., 3:]) == 0, "the padding channels are not zero"


# ------------------------------------------------------------------------------------------------ global mean, feature statistics
@pytest.mark.parametrize("B,pixels,c", [(3, 64, 128), (1, 64, 2048), (2, 35, 48)])
def test_global_mean_exact(ops, B, pixels, c):
    g = torch.Generator().manual_seed(B + pixels + c)
    x = torch.randint(-1000, 1001, (B, pixels, c), generator=g).double()
    if pixels != 64:      # a divisor that is no power of two: make every sum a multiple of it
        x[:, 0] -= x.sum(1) % pixels
    want = X.f32(x.sum(1) / pixels)
    X.assert_same_bits(ops.global_mean(X.f32(x).cuda()), want, f"global_mean {(B, pixels, c)}")


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 17])
def test_feature_stats_exact(ops, n, d):
    """two calls into the same state: integers in [-50, 50], every sum far below 2^53"""
    g = torch.Generator().manual_seed(n + d)
    total = torch.zeros(d, dtype=torch.float64, device="cuda")
    cov = torch.zeros(d, d, dtype=torch.float64, device="cuda")
    want_total, want_cov = torch.zeros(d, dtype=torch.float64), torch.zeros(d, d, dtype=torch.float64)
    for call in range(2):
        f = torch.randint(-50, 51, (n, d), generator=g).float()
        ops.feature_stats(f.cuda(), total, cov)
        want_total += f.double().sum(0)
        want_cov += f.double().t() @ f.double()
    assert torch.equal(total.cpu(), want_total), "column sums"
    got = cov.cpu()
    assert torch.equal(got, want_cov), f"cov_sum: {int((got != want_cov).sum())} of {d * d} elements differ"
